"""Where is the geometry?  The density of a trained NeRF_sigma at points that do not come from rays: a point list, or the nodes of a grid --
what mesh extraction, occupancy visualisation and point-cloud export start from -- and the surface itself, extracted on the device.

    sigma_points(model, xyz)                      [n]           sigma at xyz [n,3]
    sigma_grid(model, xs, ys, zs)                 [nz, ny, nx]  sigma at (xs[ix], ys[iy], zs[iz]); the axes need not be uniform
    density_grid(model, lo, hi, resolution)       a DensityGrid: sigma on torch.linspace axes, .occupied(threshold) -> [m,3] point cloud and
                                                  .mesh(threshold) -> a Mesh (vertices [V,3], faces [F,3] int32, normals [V,3]; .save_ply(path))
    extract_mesh(model, lo, hi, resolution, threshold)      density_grid(...).mesh(threshold); keep_largest=True: its .largest()
    Mesh.parts()                                  a MeshParts: count, vertex_part [V], face_part [F], n_vertices [K], n_faces [K]
    Mesh.largest(n=1) / .drop_small(min_faces) / .select(keep)      a new Mesh without the floaters: whole parts removed, rows and order kept
    feature_points(model, xyz, dirs)              ([n,64], [n]) the 64 rgb features and sigma at xyz seen from dirs [n,3]; one launch, full walk
    point_colors(model, decoder, style, xyz, dirs)          [n,3] in [0,1]: the features decoded by the cross-ray decoder under one appearance
    Mesh.colorize(model, decoder, style, dirs=None)         a new Mesh with colors [V,3] (dirs None: -normals); save_ply writes red green blue
    Mesh.simplify(cell, lo=None, hi=None)         a new Mesh with one vertex per occupied cell of a grid of `cell`-sized cells (vertex clustering);
                                                  extract_mesh(..., simplify_cell=c) ends with it
    Mesh.smooth(steps=10, lam=0.5, mu=-0.53)      a new Mesh after Taubin's lambda | mu smoothing, normals recomputed from the smoothed faces;
                                                  extract_mesh(..., smooth_steps=s) ends with it
    Mesh.recompute_normals()                      a new Mesh with area-weighted normals derived from its faces (a mesh that had none included)
    Views(Ks, c2ws, sizes)                        N posed pinhole views (scene.prepare_scene's Ks / poses as they are): the device tables, .pack / .split
    Mesh.depth_maps(views)                        a list of [H,W] float32 depths of the mesh in the views, +inf where it does not cover
    photo_colors(vertices, photos, views, ...)    ([n,3], [n]) colours of points by reprojection of posed photos, and the views that counted
    Mesh.colorize_from_photos(photos, views)      a new Mesh with the colours of the photographs: z-buffer, project, test, sample, average

One launch each (include/crnerf_geometry.h): the coordinates are all that is read, the embedding is built in registers and the weight stream is
walked up to the sigma head only.  `model` is a NeRF_sigma; its packed_weights(precision) is the pack.  precision "f32" or "bf16".
The mesh (include/crnerf_mesh.h): marching tetrahedra on the Kuhn split, watertight by construction, shared vertices, faces oriented out of the
dense region, the same bytes on every run; count, one read-back of the two totals, emit.
The parts (include/crnerf_mesh_parts.h): connected components by shared vertex, labelled by a lock-free union-find on the device, ids ascending
in the part's smallest vertex id; a filtered mesh is the original minus whole parts -- rows copied byte for byte, order kept, ids renumbered --
and again the same bytes on every run.  One read-back for the labels (K), one for a selection (V', F').
Simplification (csrc/crnerf_mesh_simplify.h): the mesh above follows the sampling grid, about six triangles per surface cell; vertex clustering
makes it follow a cell size of the caller's -- one vertex per occupied cell at the members' mean (exact integer sums: the same bytes on every
run), collapsed and duplicate faces dropped, normals and colours averaged.  Count, one read-back (V', F'), emit.  The order of a pipeline:
floaters first, then simplify, then colorize (or colorize first: the colours are averaged).
Smoothing and face normals (csrc/crnerf_mesh_smooth.h): the extracted surface carries the density's noise and a simplified one the blocks of
its cells; a few steps of Taubin's lambda | mu smoothing take both out without the shrinkage of plain Laplacian smoothing.  The adjacency is
built once a call, every pass is a gather over it; positions on a 2^30 integer lattice and neighbour sums in 64-bit integers -- the same bytes
on every run, whatever the order of the faces.  Normals are then re-derived from the faces, area-weighted, from integer sums again.  One
read-back, of the bounding box.  The order of a pipeline: floaters, simplify, smooth, colorize.
Photo colours (csrc/crnerf_mesh_photo.h): colorize decodes features under one style image; colorize_from_photos gives the mesh the colours of
the posed photographs themselves -- every vertex is projected into every photo, the views in which it is occluded (a z-buffer of the mesh per
view, drawn first) or faces away are dropped, and what the others see is averaged, from integer sums: the same bytes on every run.  No
read-back.  The order of a pipeline: floaters, simplify, smooth, then either colorize.
Inference only; GPU tensors only: like every op of the package there is no CPU fallback.

Domain: |coordinate| < 64.  Below it the kernels' embedding is the routine the stand-alone posenc uses (which switches to ocml's sincosf there);
the fused routine degrades beyond 200.  sigma_grid and density_grid refuse an axis or a bound outside the domain (the axes are small: the check
reads them back); sigma_points does not check its points.
"""
import math
import struct

import numpy as np
import torch

from . import ops

DOMAIN = 64.0      # |coordinate| must stay below it


class DensityGrid:
    """sigma [nz, ny, nx] and the axes it was sampled on (device tensors)."""
    __slots__ = ("sigma", "xs", "ys", "zs")

    def __init__(self, sigma, xs, ys, zs):
        self.sigma, self.xs, self.ys, self.zs = sigma, xs, ys, zs

    @torch.no_grad()
    def occupied(self, threshold):
        """[m,3]: the scene coordinates (x, y, z) of the nodes with sigma > threshold, in the grid's memory order (z slowest)."""
        iz, iy, ix = torch.nonzero(self.sigma > threshold, as_tuple=True)
        return torch.stack((self.xs[ix], self.ys[iy], self.zs[iz]), dim=1)

    @torch.no_grad()
    def mesh(self, threshold, normals=True):
        """The surface sigma == threshold as a Mesh: the nodes with sigma > threshold are inside and the faces look away from them.  The axes must be
        strictly increasing and the threshold a number (ValueError otherwise; the axes are small: the check reads them back)."""
        threshold = float(threshold)
        if math.isnan(threshold):
            raise ValueError("crnerf_amd.geometry: mesh: the threshold is NaN")
        for t, n in ((self.xs, "xs"), (self.ys, "ys"), (self.zs, "zs")):
            _check_increasing(t, n)
        return Mesh(*ops.mesh_grid(self.sigma, self.xs, self.ys, self.zs, threshold, normals=normals))


class Mesh:
    """An indexed triangle mesh: vertices [V,3] float32, faces [F,3] int32 (vertex ids, counter-clockwise seen from outside the dense region),
    normals [V,3] float32 (unit length, or zero where the density gradient vanishes) or None, colors [V,3] float32 in [0,1] (colorize) or None.
    Every method returns a new Mesh and leaves this one as it is.  Order of a pipeline: floaters first (largest / drop_small / select), then
    simplify, then smooth, then colorize -- or colorize before simplify, which averages the colours it is handed; smooth keeps them."""
    __slots__ = ("vertices", "faces", "normals", "colors")

    def __init__(self, vertices, faces, normals=None, colors=None):
        self.vertices, self.faces, self.normals, self.colors = vertices, faces, normals, colors

    @torch.no_grad()
    def colorize(self, model, decoder, style_feature, dirs=None, precision="f32"):
        """A new Mesh with colors [V,3] float32 in [0,1]: point_colors at the vertices (same vertices, faces and normals, not copied).
        dirs [V,3]: the view direction per vertex; None: -normals, the viewer looking straight at the surface (a mesh without normals: ValueError).
        A zero normal (the density gradient vanishes) gives a zero direction, which is defined: the embedding of (0, 0, 0).  The colours depend
        on the set of vertices decoded together (point_colors): colorize after removing floaters, not before, if they are to be the clean mesh's."""
        if dirs is None:
            if self.normals is None:
                raise ValueError("crnerf_amd.geometry: colorize: the mesh has no normals to look along; pass dirs [V,3]")
            dirs = -self.normals
        return Mesh(self.vertices, self.faces, self.normals, point_colors(model, decoder, style_feature, self.vertices, dirs, precision=precision))

    @torch.no_grad()
    def parts(self):
        """The connected parts of the mesh as a MeshParts (include/crnerf_mesh_parts.h: parts by shared vertex, ids ascending in the part's
        smallest vertex id).  Labelled and measured on the device; one read-back, of the number of parts."""
        return MeshParts(*ops.mesh_parts(self.faces, self.vertices.shape[0]))

    @torch.no_grad()
    def select(self, keep, parts=None):
        """A new Mesh of the parts `keep` names: a bool / uint8 [K] tensor, or a sequence of part ids.  Kept rows are the original rows, in their
        original order, ids renumbered; normals=None stays None.  parts=: the MeshParts of this mesh, when the caller has it already.  A wrong
        length, a wrong dtype or an id outside [0, K): ValueError."""
        if torch.is_tensor(keep):
            if keep.dtype not in (torch.bool, torch.uint8):      # before any device work
                raise ValueError("crnerf_amd.geometry: select: keep must be a bool or uint8 tensor, got %s" % keep.dtype)
            if keep.dim() != 1:
                raise ValueError("crnerf_amd.geometry: select: keep must be [K], got %s" % (tuple(keep.shape),))
            ids = None
        else:
            try:
                ids = [int(i) for i in keep]
                exact = all(i == k for i, k in zip(ids, keep))
            except (TypeError, ValueError):
                ids, exact = None, False
            if not exact:
                raise ValueError("crnerf_amd.geometry: select: keep must be a bool / uint8 [K] tensor or a sequence of part ids")
            if any(i < 0 for i in ids):
                raise ValueError("crnerf_amd.geometry: select: the part id %d is negative" % min(ids))
        parts = _parts_of(self, parts)
        K = parts.count
        if ids is None:
            if keep.shape[0] != K:
                raise ValueError("crnerf_amd.geometry: select: keep has %d entries for %d parts" % (keep.shape[0], K))
            keep = keep.to(self.faces.device).contiguous()
        else:
            if ids and max(ids) >= K:
                raise ValueError("crnerf_amd.geometry: select: the part id %d is outside [0, %d)" % (max(ids), K))
            keep = torch.zeros(K, dtype=torch.uint8, device=self.faces.device)
            if ids:
                keep[torch.tensor(ids, dtype=torch.int64, device=keep.device)] = 1
        return Mesh(*_select(self, parts, keep))

    @torch.no_grad()
    def largest(self, n=1, parts=None):
        """A new Mesh of the n parts with the most faces (ties go to the smaller part id); the rows stay in their original order.  Ranked on the
        device."""
        n = int(n)
        if n < 0:
            raise ValueError("crnerf_amd.geometry: largest: n must not be negative, got %d" % n)
        parts = _parts_of(self, parts)
        keep = torch.zeros(parts.count, dtype=torch.uint8, device=self.faces.device)
        if parts.count and n:
            order = torch.sort(parts.n_faces, descending=True, stable=True).indices      # stable: equal sizes stay in id order
            keep[order[:n]] = 1
        return Mesh(*_select(self, parts, keep))

    @torch.no_grad()
    def drop_small(self, min_faces, parts=None):
        """A new Mesh of the parts with at least min_faces faces."""
        parts = _parts_of(self, parts)
        return Mesh(*_select(self, parts, (parts.n_faces >= int(min_faces)).to(torch.uint8)))

    @torch.no_grad()
    def simplify(self, cell, lo=None, hi=None):
        """A new Mesh simplified by vertex clustering (csrc/crnerf_mesh_simplify.h states every rule): the box [lo, hi] is cut into cells of size
        `cell` -- a positive float, or (cx, cy, cz) --, n_a = max(1, ceil((hi_a - lo_a) / cell_a)) of them on axis a, and the vertices of a cell
        become one vertex at their mean.  A face whose corners fall into fewer than three cells is dropped; of the faces over the same three cells
        the first stays; the kept faces keep their order and orientation.  Normals and colours are carried when present -- the normalised mean and
        the mean of the members' --, None stays None.  lo / hi: 3-sequences; None: the vertices' bounding box (one extra read-back, of six floats);
        a vertex outside the box belongs to the nearest border cell.  An empty mesh gives an empty mesh, without a read-back.
        Order: floaters first (largest / drop_small: a small cell can merge a floater into the surface it hovers over), then simplify, then
        colorize -- or colorize first and let simplify average the colours.  A cell that no kept face uses leaves an unused vertex: drop_small(1)
        removes those.  ValueError: a cell that is not finite and > 0, a bound that is not finite, hi < lo, more than 2^20 cells on an axis or
        more than 2^31 - 1 in all."""
        what = "crnerf_amd.geometry: simplify"
        try:
            cells = [float(cell)] * 3 if not hasattr(cell, "__len__") else [float(c) for c in cell]
        except (TypeError, ValueError):
            cells = []
        if len(cells) != 3:
            raise ValueError("%s: cell must be a positive float or a 3-sequence of them, got %r" % (what, cell))
        if not all(math.isfinite(c) and c > 0.0 for c in cells):
            raise ValueError("%s: cell must be finite and > 0, got %r" % (what, cell))
        bounds = []
        for name, b in (("lo", lo), ("hi", hi)):
            if b is not None:
                try:
                    b = [float(x) for x in b]
                except (TypeError, ValueError):
                    b = []
                if len(b) != 3 or not all(math.isfinite(x) for x in b):
                    raise ValueError("%s: %s must be a 3-sequence of finite floats" % (what, name))
            bounds.append(b)
        lo, hi = bounds
        if lo is not None and hi is not None:      # before the device is needed
            n = _cluster_cells(lo, hi, cells, what)
        if self.vertices.shape[0] == 0:
            empty = self.vertices.new_empty((0, 3))
            return Mesh(empty, self.faces.new_empty((0, 3)), None if self.normals is None else empty.clone(),
                        None if self.colors is None else empty.clone())
        if lo is None or hi is None:
            box = torch.stack((self.vertices.min(dim=0).values, self.vertices.max(dim=0).values)).tolist()
            lo, hi = box[0] if lo is None else lo, box[1] if hi is None else hi
            if not all(math.isfinite(x) for x in lo + hi):
                raise ValueError("%s: the vertices' bounding box is not finite; pass lo and hi" % what)
            n = _cluster_cells(lo, hi, cells, what)
        v, f, nrm, col, _ = ops.mesh_cluster(self.vertices, self.faces, lo, cells, n, normals=self.normals, colors=self.colors)
        return Mesh(v, f, nrm, col)

    @torch.no_grad()
    def smooth(self, steps=10, lam=0.5, mu=-0.53, pin_border=True):
        """A new Mesh after `steps` steps of Taubin's lambda | mu smoothing (csrc/crnerf_mesh_smooth.h states every rule): per step a pass that
        moves every vertex by lam times the way to the mean of its neighbours and a pass with mu, which undoes the shrinkage -- the noise of a
        trained density and the blocks of simplify go, the shape stays.  A neighbour counts once per face that joins the two.  Vertices without
        a face stay where they are, and with pin_border so do the vertices of an open border.  Same faces and colours (not copied); normals,
        when the mesh has them, are recomputed from the smoothed faces (recompute_normals), None stays None.  The positions live on a 2^30
        lattice over a box around the bounding box (one read-back, of six floats): the same bytes on every run, whatever the order of the
        faces.  steps = 0 returns this mesh; an empty mesh gives an empty mesh, without a read-back.
        Order: floaters first, then simplify, then smooth, then colorize -- colorize(dirs=None) then looks along normals that belong to the
        surface.  ValueError: steps that is not an int >= 0, a lam or mu that is not finite or has |w| > 2, a bounding box that is not finite."""
        what = "crnerf_amd.geometry: smooth"
        if isinstance(steps, bool) or not isinstance(steps, int) or not 0 <= steps <= 65536:
            raise ValueError("%s: steps must be an int in [0, 65536], got %r" % (what, steps))
        weights = []
        for name, w in (("lam", lam), ("mu", mu)):
            try:
                w = float(w)
            except (TypeError, ValueError):
                w = math.nan
            if not (math.isfinite(w) and abs(w) <= 2.0):
                raise ValueError("%s: %s must be a finite float with |%s| <= 2, got %r" % (what, name, name, lam if name == "lam" else mu))
            weights.append(w)
        if steps == 0:
            return self
        if self.vertices.shape[0] == 0:
            empty = self.vertices.new_empty((0, 3))
            return Mesh(empty, self.faces, None if self.normals is None else empty.clone(), self.colors)
        lo, e = _lattice_box(self.vertices, what)
        v = ops.mesh_smooth(self.vertices, self.faces, lo, 29 - e, steps, weights[0], weights[1], pin_border=bool(pin_border))
        nrm = None if self.normals is None else ops.mesh_vertex_normals(v, self.faces, 44 - 2 * e)
        return Mesh(v, self.faces, nrm, self.colors)

    @torch.no_grad()
    def recompute_normals(self):
        """A new Mesh whose normals are derived from its faces (csrc/crnerf_mesh_smooth.h, Face normals per vertex): per vertex the
        area-weighted mean of the normals of its faces, of unit length, and zero for a vertex no face uses.  The faces are counter-clockwise
        seen from outside, so these point the way an extracted mesh's density-gradient normals do.  It works on a mesh that had none -- one a
        caller built, which colorize(dirs=None) could not look at -- and replaces the averaged normals of simplify.  Same vertices, faces and
        colours (not copied); one read-back, of six floats."""
        if self.vertices.shape[0] == 0:
            return Mesh(self.vertices, self.faces, self.vertices.new_empty((0, 3)), self.colors)
        _, e = _lattice_box(self.vertices, "crnerf_amd.geometry: recompute_normals")
        return Mesh(self.vertices, self.faces, ops.mesh_vertex_normals(self.vertices, self.faces, 44 - 2 * e), self.colors)

    @torch.no_grad()
    def depth_maps(self, views, z_near=1e-3):
        """The z-buffer of this mesh in every view of `views` (a Views; csrc/crnerf_mesh_photo.h states every rule): a list of [H,W] float32
        tensors -- views of one flat buffer, views.split's --, the depth along the optical axis of the nearest face at each pixel and +inf
        where the mesh does not cover.  Both orientations of a face are drawn; a face with a corner nearer than z_near (or behind the camera)
        is not drawn at all: there is no near-plane clipping.  An empty mesh gives maps of +inf."""
        return views.split(_zbuffer(self, views, z_near))

    @torch.no_grad()
    def colorize_from_photos(self, photos, views, occlusion=True, facing=True, depth_tol=0.02, z_near=1e-3, fallback=None):
        """A new Mesh with colors [V,3] float32 in [0,1] taken from posed photographs (same vertices, faces and normals, not copied):
        photo_colors at the vertices.  photos: a list of uint8 [H,W,3] arrays or tensors, one per view of `views` (a Views), or views.pack's
        buffer.  occlusion=True draws the z-buffer of THIS mesh first (depth_maps) and drops a view in which the vertex lies behind it by more
        than the factor 1 + depth_tol: a smaller tolerance rejects grazing views, in which the depth changes fast across a pixel; a larger one
        lets background leak onto the surface at silhouettes.  facing=True hands the normals over when the mesh has them: a view the surface
        faces away from does not count.  z_near: a vertex (and for the z-buffer a face with a corner) nearer to a camera than this is ignored
        by that camera.  A vertex no view sees takes `fallback` [V,3] if given, else the mesh's existing colour if it has colours, else 0.5
        grey.  An empty mesh gives an empty mesh, without a launch.  Order: floaters, simplify, smooth, then this."""
        V = self.vertices.shape[0]
        if fallback is not None and (not torch.is_tensor(fallback) or tuple(fallback.shape) != (V, 3)):
            raise ValueError("crnerf_amd.geometry: colorize_from_photos: fallback must be a [%d,3] tensor" % V)
        if V == 0:
            _check_views(views, "colorize_from_photos")
            return Mesh(self.vertices, self.faces, self.normals, self.vertices.new_empty((0, 3)))
        depths = _zbuffer(self, views, z_near) if occlusion else None
        colors, seen = photo_colors(self.vertices, photos, views, normals=self.normals if facing else None, depths=depths, depth_tol=depth_tol,
                                    z_near=z_near)
        rest = fallback if fallback is not None else self.colors
        rest = torch.full_like(colors, 0.5) if rest is None else rest.to(colors.device, torch.float32)
        return Mesh(self.vertices, self.faces, self.normals, torch.where((seen > 0)[:, None], colors, rest))

    def save_ply(self, path):
        """Binary little-endian PLY: float32 x y z (and nx ny nz when the mesh has normals, then uchar red green blue when it has colors:
        (c.clamp(0, 1) * 255) truncated) per vertex, `uchar int` vertex_indices per face.  Copies to the host itself; needs no third-party package."""
        v = self.vertices.detach().to("cpu", torch.float32)
        f = self.faces.detach().to("cpu", torch.int32)
        if v.dim() != 2 or v.shape[1] != 3 or f.dim() != 2 or f.shape[1] != 3:
            raise ValueError("crnerf_amd.geometry: save_ply expects vertices [V,3] and faces [F,3], got %s and %s" % (tuple(v.shape), tuple(f.shape)))
        props = ["x", "y", "z"]
        if self.normals is not None:
            n = self.normals.detach().to("cpu", torch.float32)
            if tuple(n.shape) != tuple(v.shape):
                raise ValueError("crnerf_amd.geometry: save_ply: normals %s do not match vertices %s" % (tuple(n.shape), tuple(v.shape)))
            v = torch.cat((v, n), dim=1)
            props += ["nx", "ny", "nz"]
        vrows = _little_endian(v.contiguous())
        uprops = []
        if self.colors is not None:
            c = self.colors.detach().to("cpu", torch.float32)
            if tuple(c.shape) != (v.shape[0], 3):
                raise ValueError("crnerf_amd.geometry: save_ply: colors %s do not match %d vertices" % (tuple(c.shape), v.shape[0]))
            # the video path's rule (video.render_video): clamp to [0,1], times 255, truncated
            vrows = torch.cat((vrows.view(torch.uint8).reshape(v.shape[0], 4 * len(props)), (c.clamp(0, 1) * 255).to(torch.uint8)), dim=1)
            uprops = ["red", "green", "blue"]
        header = "".join(["ply\nformat binary_little_endian 1.0\ncomment crnerf_amd.geometry\nelement vertex %d\n" % v.shape[0]]
                         + ["property float %s\n" % p for p in props] + ["property uchar %s\n" % p for p in uprops]
                         + ["element face %d\nproperty list uchar int vertex_indices\nend_header\n" % f.shape[0]])
        rows = torch.empty(f.shape[0], 13, dtype=torch.uint8)      # one count byte, three little-endian int32
        rows[:, 0] = 3
        rows[:, 1:] = _little_endian(f.contiguous()).view(torch.uint8).reshape(-1, 12)
        with open(path, "wb") as out:
            out.write(header.encode("ascii"))
            out.write(vrows.numpy().tobytes())
            out.write(rows.numpy().tobytes())


class Views:
    """N posed pinhole views as the three device tables of csrc/crnerf_mesh_photo.h, built once.  Ks: N 3x3 intrinsics (fx = K[0][0],
    fy = K[1][1], cx = K[0][2], cy = K[1][2]); c2ws: N 3x4 camera-to-world poses in the training rays' convention (x right, y up, looking
    along -z) -- datasets.scene.prepare_scene's sc.Ks / sc.poses go in as they are, float64 is kept --; sizes: N (W, H) pairs.  The views lie
    one behind the other in a flat buffer of total_pixels pixels.  ValueError, before the device is needed: wrong shapes, an entry that is
    not finite, a W or H outside [2, 16384].
    .n, .sizes [(W, H)], .offsets [int], .total_pixels; .cams [N,16] float64, .dims [N,2] int32, .offset_table [N] int64 on the device;
    .split(flat) -> the list of [H,W] (or [H,W,3]) views of a flat [total_pixels] (or [total_pixels,3]) buffer; .pack(photos) -> the flat
    uint8 [total_pixels,3] device buffer of a list of uint8 [H,W,3] photos."""
    __slots__ = ("n", "sizes", "offsets", "total_pixels", "cams", "dims", "offset_table")

    def __init__(self, Ks, c2ws, sizes, device="cuda"):
        what = "crnerf_amd.geometry: Views"
        try:
            K, P = _host_f64(Ks), _host_f64(c2ws)
            sizes = [tuple(s) for s in sizes]
            wh = [(int(w), int(h)) for w, h in sizes]
            exact = all(w == a and h == b for (w, h), (a, b) in zip(wh, sizes))
        except (TypeError, ValueError, RuntimeError):
            raise ValueError("%s expects Ks as N 3x3 intrinsics, c2ws as N 3x4 poses and sizes as N (W, H) pairs of ints" % what) from None
        N = len(wh)
        if N == 0 and K.numel() == 0 and P.numel() == 0:      # no view: the tables are empty
            K, P = K.reshape(0, 3, 3), P.reshape(0, 3, 4)
        if K.dim() != 3 or tuple(K.shape) != (N, 3, 3) or tuple(P.shape) != (N, 3, 4) or not exact:
            raise ValueError("%s expects Ks [N,3,3], c2ws [N,3,4] and N (W, H) pairs of ints, got %s, %s and %d sizes"
                             % (what, tuple(K.shape), tuple(P.shape), N))
        if not (bool(torch.isfinite(K).all()) and bool(torch.isfinite(P).all())):
            raise ValueError("%s: an entry of Ks or c2ws is not finite" % what)
        for w, h in wh:
            if not (2 <= w <= 16384 and 2 <= h <= 16384):
                raise ValueError("%s: a view of %d x %d; W and H must lie in [2, 16384]" % (what, w, h))
        cams = torch.cat((K[:, 0, 0:1], K[:, 1, 1:2], K[:, 0, 2:3], K[:, 1, 2:3], P[:, :, :3].reshape(N, 9), P[:, :, 3]), dim=1)
        offsets, total = [], 0
        for w, h in wh:
            offsets.append(total)
            total += w * h
        self.n, self.sizes, self.offsets, self.total_pixels = N, wh, offsets, total
        self.cams = cams.contiguous().to(device)
        self.dims = torch.tensor(wh, dtype=torch.int32).reshape(N, 2).to(device)
        self.offset_table = torch.tensor(offsets, dtype=torch.int64).to(device)

    def split(self, flat):
        """The views of a flat buffer [total_pixels] or [total_pixels, C] as a list of [H,W] or [H,W,C] tensors (views of it, not copies)."""
        if not torch.is_tensor(flat) or flat.dim() not in (1, 2) or flat.shape[0] != self.total_pixels:
            raise ValueError("crnerf_amd.geometry: Views.split expects a [%d] or [%d,C] tensor" % (self.total_pixels, self.total_pixels))
        return [flat[o:o + w * h].reshape((h, w) + tuple(flat.shape[1:])) for o, (w, h) in zip(self.offsets, self.sizes)]

    def pack(self, photos):
        """One flat uint8 [total_pixels,3] device buffer of the photos: a list of N uint8 [H,W,3] arrays or tensors, on the host or the
        device.  ValueError: a count, dtype or shape that does not match its view."""
        what = "crnerf_amd.geometry: Views.pack"
        photos = list(photos)
        if len(photos) != self.n:
            raise ValueError("%s: %d photos for %d views" % (what, len(photos), self.n))
        rows = []
        for k, (img, (w, h)) in enumerate(zip(photos, self.sizes)):
            t = torch.as_tensor(img)
            if t.dtype != torch.uint8 or tuple(t.shape) != (h, w, 3):
                raise ValueError("%s: photo %d must be uint8 [%d,%d,3] ([H,W,3] of its view), got %s %s" % (what, k, h, w, t.dtype, tuple(t.shape)))
            rows.append(t)
        dev = self.cams.device
        if not rows:
            return torch.empty(0, 3, dtype=torch.uint8, device=dev)
        if all(t.device.type == "cpu" for t in rows):      # host photos: one buffer on the host, one upload
            return torch.cat([t.reshape(-1, 3) for t in rows]).to(dev)
        return torch.cat([t.reshape(-1, 3).to(dev) for t in rows])


def _host_f64(a):
    """A tensor, an array or a (nested) sequence of either as one float64 tensor on the host; float64 input keeps its bits."""
    if torch.is_tensor(a):
        return a.detach().to("cpu", torch.float64)
    if isinstance(a, (list, tuple)) and len(a) and all(torch.is_tensor(t) for t in a):
        return torch.stack([t.detach().to("cpu", torch.float64) for t in a])
    return torch.from_numpy(np.array(a, dtype=np.float64))


def _check_views(views, what):
    if not isinstance(views, Views):
        raise ValueError("crnerf_amd.geometry: %s: views must be a geometry.Views" % what)
    return views


def _zbuffer(mesh, views, z_near):
    """The flat depth buffer of the mesh in the views."""
    v = _check_views(views, "depth_maps")
    return ops.mesh_zbuffer(mesh.vertices, mesh.faces, v.cams, v.dims, v.offset_table, v.total_pixels, z_near)


@torch.no_grad()
def photo_colors(vertices, photos, views, normals=None, depths=None, depth_tol=0.02, z_near=1e-3):
    """(colors [n,3] float32 in [0,1], n_views [n] int32) of the points vertices [n,3] by reprojection of posed photos (csrc/crnerf_mesh_photo.h
    states every rule): every point is projected into every view of `views` (a Views); a view counts when the point is at least z_near in front
    of it, inside the photo, faces the camera (normals [n,3] given and not zero) and is not occluded (depths given); the counting views'
    bilinear samples are averaged.  Zeros, and n_views 0, where no view counts.  photos: a list of uint8 [H,W,3] arrays, as for views.pack, or
    the packed buffer.  depths: the flat buffer or the list of Mesh.depth_maps, or None for no occlusion test -- depths along the optical
    axis, NOT the renderer's along-ray depths.  depth_tol: a point may lie behind the z-buffer by the factor 1 + depth_tol; a smaller
    tolerance rejects grazing views, a larger one lets background leak at silhouettes."""
    v = _check_views(views, "photo_colors")
    packed = photos if torch.is_tensor(photos) else v.pack(photos)
    if depths is not None and not torch.is_tensor(depths):
        depths = list(depths)
        if len(depths) != v.n or any(not torch.is_tensor(d) or tuple(d.shape) != (h, w) for d, (w, h) in zip(depths, v.sizes)):
            raise ValueError("crnerf_amd.geometry: photo_colors: depths must be the flat buffer or the list of [H,W] maps of Mesh.depth_maps")
        depths = torch.cat([d.reshape(-1) for d in depths]) if depths else torch.empty(0, dtype=torch.float32, device=v.cams.device)
    return ops.mesh_photo_colors(vertices, normals, packed, depths, v.cams, v.dims, v.offset_table, v.total_pixels, z_near, depth_tol)


class MeshParts:
    """The connected parts of a Mesh: count K, vertex_part [V] int32, face_part [F] int32 (-1 for a face with an id outside [0, V)), and the sizes
    n_vertices [K], n_faces [K] int32 (device tensors).  Part ids ascend in the smallest vertex id of the part."""
    __slots__ = ("vertex_part", "face_part", "n_vertices", "n_faces")

    def __init__(self, vertex_part, face_part, n_vertices, n_faces):
        self.vertex_part, self.face_part, self.n_vertices, self.n_faces = vertex_part, face_part, n_vertices, n_faces

    @property
    def count(self):
        return int(self.n_faces.shape[0])


def _parts_of(mesh, parts):
    """The caller's MeshParts, held to the mesh; None: the mesh is labelled now."""
    if parts is None:
        return mesh.parts()
    if not isinstance(parts, MeshParts):
        raise ValueError("crnerf_amd.geometry: parts must be the MeshParts of this mesh (Mesh.parts())")
    if parts.vertex_part.shape[0] != mesh.vertices.shape[0] or parts.face_part.shape[0] != mesh.faces.shape[0]:
        raise ValueError("crnerf_amd.geometry: parts labels %d vertices and %d faces, the mesh has %d and %d"
                         % (parts.vertex_part.shape[0], parts.face_part.shape[0], mesh.vertices.shape[0], mesh.faces.shape[0]))
    return parts


def _cluster_cells(lo, hi, cell, what):
    """n_a = max(1, ceil((hi_a - lo_a) / cell_a)) in Python floats, held to what the clustering grid may be."""
    for a in range(3):
        if hi[a] < lo[a]:
            raise ValueError("%s: hi must not lie below lo, got lo = %r and hi = %r" % (what, lo, hi))
    n = []
    for a in range(3):
        q = (hi[a] - lo[a]) / cell[a]
        if not q <= 2 ** 20:      # (an infinite quotient too)
            raise ValueError("%s: cell = %r cuts the box into more than 2^20 cells on an axis" % (what, cell))
        n.append(max(1, math.ceil(q)))
    if n[0] * n[1] * n[2] > 2 ** 31 - 1:
        raise ValueError("%s: cell = %r cuts the box into %d x %d x %d cells, more than 2^31 - 1 in all" % (what, cell, n[0], n[1], n[2]))
    return n


def _lattice_box(vertices, what):
    """(lo, e) of the smoothing lattice (csrc/crnerf_mesh_smooth.h, Fixed point): E = the largest extent of the bounding box (0 counts as 1),
    e = ceil(log2(E)) -- from the exponent of E, not from a rounded logarithm --, lo_a = (min_a + max_a) / 2 - 2^e in Python floats; the caller
    passes k = 29 - e and k2 = 44 - 2 e.  One read-back, of six floats."""
    ops._parts_input(vertices, "vertices", what, torch.float32, cols=3, on_device=False)
    # (over the rows of the transposed copy: a reduction along the short side of a [V,3] tensor takes five times as long, profiles/r25)
    box = torch.stack(torch.aminmax(vertices.t().contiguous(), dim=1)).tolist()
    if not all(math.isfinite(x) for x in box[0] + box[1]):
        raise ValueError("%s: the vertices' bounding box is not finite" % what)
    E = max(box[1][a] - box[0][a] for a in range(3))
    m, x = math.frexp(E if E > 0.0 else 1.0)      # E = m 2^x, 0.5 <= m < 1
    e = x - 1 if m == 0.5 else x
    if not -71 <= e <= 126:      # k = 29 - e must lie in [-100, 100], and 2^e in float32
        raise ValueError("%s: the bounding box's largest extent %g is outside [2^-71, 2^126]" % (what, E))
    return [(box[0][a] + box[1][a]) / 2 - math.ldexp(1.0, e) for a in range(3)], e


def _select(mesh, parts, keep):
    v, f, n = ops.mesh_select(mesh.vertices, mesh.faces, mesh.normals, parts.vertex_part, parts.face_part, keep)
    # the colours of the kept vertices: a vertex stays when its part does, rows in their original order (include/crnerf_mesh_parts.h, Selection)
    c = None if mesh.colors is None else mesh.colors[keep.bool()[parts.vertex_part.long()]]
    return v, f, n, c


_HOST_IS_LITTLE =struct.pack("=H", 1) == struct.pack("<H", 1)


def _little_endian(t):
    """The tensor with its 4-byte elements in little-endian byte order (as it is on a little-endian host)."""
    return t if _HOST_IS_LITTLE else t.view(torch.uint8).reshape(-1, 4).flip(1).reshape(-1).view(t.dtype).reshape(t.shape)


def _check_axis(t, name):
    """Rank, then domain -- wherever the axis lives: the refusal needs no device."""
    ops._sigma_input(t, name, "sigma_grid", on_device=False)
    if t.numel() > 0:
        worst = float(t.abs().max())
        if not worst < DOMAIN:          # (a NaN is refused too)
            raise ValueError("crnerf_amd.geometry: the axis %s reaches |v| = %g; the density query is defined for |v| < %g" % (name, worst, DOMAIN))


def _check_increasing(t, name):
    """The orientation of the faces, and t in [0, 1] meaning `between the nodes`, rest on axes that rise."""
    ops._sigma_input(t, name, "mesh", on_device=False)
    if t.numel() > 1 and not bool((t[1:] > t[:-1]).all()):      # (a NaN is refused too)
        raise ValueError("crnerf_amd.geometry: mesh: the axis %s is not strictly increasing" % name)


@torch.no_grad()
def sigma_points(model, xyz, precision="f32"):
    """sigma [n] at xyz [n,3] (float32, contiguous, on the GPU).  Domain |coordinate| < 64: documented, not checked."""
    name = ops._sigma_query_core(precision, "sigma_points")
    ops._sigma_input(xyz, "xyz", "sigma_points", points=True)
    return ops.sigma_points(model.packed_weights(name), xyz, precision=precision)


@torch.no_grad()
def feature_points(model, xyz, dirs, precision="f32"):
    """(feature [n,64], sigma [n]) at xyz [n,3] seen from dirs [n,3] (float32, contiguous, on the GPU): ops.feature_points on the model's pack.
    Domain |coordinate| < 64, points and directions: documented, not checked."""
    name = ops._sigma_query_core(precision, "feature_points")
    _check_point_features(xyz, dirs, "feature_points")
    return ops.feature_points(model.packed_weights(name), xyz, dirs, precision=precision)


@torch.no_grad()
def point_colors(model, decoder, style_feature, xyz, dirs, precision="f32"):
    """colours [n,3] float32 in [0,1] of the points xyz [n,3] seen from dirs [n,3], in the appearance of style_feature: the model's 64 rgb features
    at the points (one launch, ops.feature_points) decoded by the cross-ray decoder exactly as a rendered image's feature grid is --
    ops.crossray_decode(feature, style, decoder.decoder_tensors()), transposed and clamped.  decoder: models["decoder"], a style_net;
    style_feature: enc_a(style_img), [1,64,h,w].
    The colours depend on the SET of points decoded together: the decoder's cross-ray statistics (mean and Gram) run over the content it is
    handed, just as a pixel's colour depends on its image in this model.  Decode a mesh's vertices, or a cloud, in one call -- a chunked call
    gives every chunk its own statistics.  n == 0: [0,3], the decoder is not called.  A coloured point cloud: point_colors(..., g.occupied(t), dirs)."""
    name = ops._sigma_query_core(precision, "point_colors")
    _check_point_features(xyz, dirs, "point_colors")
    if xyz.shape[0] == 0:
        return torch.empty(0, 3, dtype=torch.float32, device=xyz.device)
    from .models.linearStyleTransfer import _pixel_major
    style_pm, _ = _pixel_major(style_feature)
    feature, _ = ops.feature_points(model.packed_weights(name), xyz, dirs, precision=precision, want_sigma=False)
    return ops.crossray_decode(feature, style_pm, decoder.decoder_tensors()).t().clamp(0.0, 1.0).contiguous()


def _check_point_features(xyz, dirs, what):
    """float32, contiguous, on the device, a direction per point: before the model is asked for its pack."""
    for t, n in ((xyz, "xyz"), (dirs, "dirs")):
        ops._sigma_input(t, n, what, points=True, on_device=False)
    if xyz.shape[0] != dirs.shape[0]:
        raise ValueError("crnerf_amd: %s: xyz has %d rows and dirs has %d; a direction per point" % (what, xyz.shape[0], dirs.shape[0]))
    for t, n in ((xyz, "xyz"), (dirs, "dirs")):
        ops._sigma_input(t, n, what, points=True)


@torch.no_grad()
def sigma_grid(model, xs, ys, zs, precision="f32", out=None):
    """sigma [nz, ny, nx] at (xs[ix], ys[iy], zs[iz]); the axes are 1-D float32 device tensors with |v| < 64 (ValueError otherwise).  out=: see
    ops.sigma_grid."""
    name = ops._sigma_query_core(precision, "sigma_grid")
    for t, n in ((xs, "xs"), (ys, "ys"), (zs, "zs")):
        _check_axis(t, n)
    for t, n in ((xs, "xs"), (ys, "ys"), (zs, "zs")):      # float32, contiguous, on the device: before the model is asked for its pack
        ops._sigma_input(t, n, "sigma_grid")
    return ops.sigma_grid(model.packed_weights(name), xs, ys, zs, precision=precision, out=out)


@torch.no_grad()
def density_grid(model, lo, hi, resolution, precision="f32"):
    """The density on the box [lo, hi] (3-sequences of floats, scene coordinates): axis a is torch.linspace(lo[a], hi[a], n[a]) with
    n = resolution (an int, or (nx, ny, nz)).  Returns a DensityGrid."""
    name = ops._sigma_query_core(precision, "density_grid")
    lo, hi = [float(v) for v in lo], [float(v) for v in hi]
    n = [int(resolution)] * 3 if isinstance(resolution, int) else [int(v) for v in resolution]
    if len(lo) != 3 or len(hi) != 3 or len(n) != 3:
        raise ValueError("crnerf_amd.geometry: density_grid expects lo and hi as 3-sequences and resolution as an int or (nx, ny, nz)")
    if min(n) < 1:
        raise ValueError("crnerf_amd.geometry: density_grid: resolution must be positive, got %s" % (n,))
    for v in lo + hi:
        if not abs(v) < DOMAIN:
            raise ValueError("crnerf_amd.geometry: density_grid: the bound %g is outside |v| < %g, the domain of the density query" % (v, DOMAIN))
    pack = model.packed_weights(name)
    dev = pack.device
    xs, ys, zs = (torch.linspace(lo[a], hi[a], n[a], dtype=torch.float32, device=dev) for a in range(3))
    return DensityGrid(ops.sigma_grid(pack, xs, ys, zs, precision=precision), xs, ys, zs)


@torch.no_grad()
def extract_mesh(model, lo, hi, resolution, threshold, precision="f32", keep_largest=False, simplify_cell=None, smooth_steps=0):
    """density_grid(model, lo, hi, resolution, precision).mesh(threshold): the surface of the box's density as a Mesh.  keep_largest=True: its
    .largest(1) -- the part with the most faces, the floaters of a trained density gone.  simplify_cell=c: then its .simplify(c), in that order
    -- extract, largest when asked, simplify (over the bounding box of what is left); None: the mesh as it is.  smooth_steps=s > 0: then its
    .smooth(s) at the default weights, the normals recomputed from the smoothed faces."""
    if math.isnan(float(threshold)):      # before the grid is paid for
        raise ValueError("crnerf_amd.geometry: mesh: the threshold is NaN")
    nothing = Mesh(torch.empty(0, 3), torch.empty(0, 3, dtype=torch.int32))
    if simplify_cell is not None:
        nothing.simplify(simplify_cell)      # a bad cell: refused before the grid is paid for
    nothing.smooth(smooth_steps)             # and bad steps
    mesh = density_grid(model, lo, hi, resolution, precision=precision).mesh(threshold)
    if keep_largest:
        mesh = mesh.largest(1)
    if simplify_cell is not None:
        mesh = mesh.simplify(simplify_cell)
    return mesh.smooth(smooth_steps) if smooth_steps > 0 else mesh

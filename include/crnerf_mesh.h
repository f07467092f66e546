/* Companion header of include/crnerf.h and include/crnerf_geometry.h: the iso-surface of a density grid as an indexed triangle mesh, extracted on
 * the device and exported from the same libcrnerf_hip.so.  A file of its own because crnerf.h and crnerf_geometry.h are pinned, text and prototype
 * count, by the tests of the rounds that wrote them.  Conventions (device pointers, `stream`, error codes, crnerf_last_error) are those of
 * crnerf.h; crnerf_abi_version() is unchanged.
 *
 * Input: sigma[nz][ny][nx] float32 (what crnerf_sigma_grid_* writes: node (ix, iy, iz) at flat index ix + nx (iy + ny iz)) and the axis arrays
 * xs[nx], ys[ny], zs[nz] (float32; strictly increasing is what the orientation rule below assumes -- not checked here).
 * Output: vertices[V][3] float32, faces[F][3] int32 (vertex ids), normals[V][3] float32.  Content AND order are fixed by the rules below: two
 * runs give the same bytes, and a C caller can predict them.
 *
 * ALGORITHM: marching tetrahedra on the Kuhn split of every cell.  No ambiguous case; the split is translation invariant, so neighbouring cells
 * agree on their shared faces and a surface that does not leave the grid is closed.
 *
 *   Inside.  A node is inside iff sigma > threshold (strictly; NaN and -inf are outside, +inf is inside).
 *   Edges.  Node p = (ix, iy, iz) owns up to seven edges p -> p + d, d in {0,1}^3 \ {0}, direction index dx + 2 dy + 4 dz - 1 (0..6).  An edge is
 *     valid if p + d lies in the grid, and active if exactly one of its ends is inside.
 *   Vertices.  One per active edge, ordered by (flat index of the owning node, direction index), ascending.  With a the owning node and b the
 *     other end: t = (threshold - sa) / (sb - sa), then x = xa + t (xb - xa) per coordinate, in float32, every operation rounded on its own (no
 *     fused multiply-add).  If t is not finite or lies outside [0, 1], t = 0.5.
 *   Tetrahedra.  A cell with origin p (ix < nx - 1, iy < ny - 1, iz < nz - 1) splits into six: tet 0..5 is the path
 *     p -> p + e_a -> p + e_a + e_b -> p + (1,1,1) with (a, b, c) = xyz, xzy, yxz, yzx, zxy, zyx.
 *   Faces of a tet.  One or three inside nodes: one triangle on the three active edges.  Two inside nodes i0 < i1 (path order), outside o0 < o1:
 *     the quad (i0 o0), (i0 o1), (i1 o1), (i1 o0) -- consecutive edges share a node.
 *   Orientation.  For increasing axes and 0 < t < 1, (v1 - v0) x (v2 - v0) points from the inside nodes towards the outside nodes: out of the
 *     dense region.  The cycle is reversed where the rule above gives the other sense; this depends on the (tet, pattern) case alone.
 *   Rotation, quad split.  Every triangle or quad is rotated so that its smallest vertex id comes first; a quad (q0, q1, q2, q3) then becomes
 *     the faces (q0, q1, q2) and (q0, q2, q3).
 *   Face order.  By (flat index of the cell's origin over the NODE grid, tet index, triangle within the tet), ascending.
 *   Degenerate triangles.  A node whose value is exactly the threshold is outside and t is 0 or 1 on its edges: zero-area triangles.  They are
 *     kept -- the topology is what is promised.
 *   Short axes.  Any axis shorter than 2: V = F = 0.
 *   Normals.  The gradient of sigma at the two end nodes (per axis: central difference, one-sided at the border, divided by the actual spacing of
 *     the axis), interpolated along the edge with the vertex's t (same two-rounding form), negated -- density rises inwards --, and divided by
 *     its length.  A length of zero (or one that is not finite) gives the zero vector.
 *
 * USE: size a workspace, count, read the two totals back (the one synchronisation), allocate, emit -- all on one stream.
 *
 * crnerf_mesh_workspace_bytes: bytes of device scratch for a grid (5 a node + 16 per 1,024 nodes + 32); 0 for an empty grid and for a shape
 *   count would refuse.  The workspace must be 16-byte aligned (CRNERF_ERR_CONFIG otherwise).  It links count to emit: emit reads what count
 *   left there (per node: the 7-bit active-edge mask and the vertex / face offsets inside its block of 1,024; per block: the 64-bit bases).
 * crnerf_mesh_count_f32: one pass over the nodes, then one single-workgroup pass over the block totals (no workgroup ever waits on another);
 *   counts[0] = V and counts[1] = F are written on the device, in stream order.
 * crnerf_mesh_emit_f32: same sigma, shape and threshold as the count call that filled `workspace`.  Writes vertices, normals (NULL: skipped) and
 *   faces.  v_cap / f_cap are the rows the buffers hold: a row at or beyond its cap is not written (normals holds v_cap rows too), so a short
 *   buffer yields a truncated mesh, never a write past it.  V > 2^31 - 1 cannot be indexed by int32 faces: split the grid.
 *
 * Refusals, on the host before any device work: a negative axis length, nx * ny * nz above 2^31 - 1, in emit a negative capacity or one above
 * 2^31 - 1 (CRNERF_ERR_SHAPE); a NULL pointer with work to do (CRNERF_ERR_NULL: sigma, workspace, counts / sigma, xs, ys, zs, workspace, vertices
 * when v_cap > 0, faces when f_cap > 0).  An empty grid or an axis shorter than 2: returns 0, launches nothing; count zeroes counts[0..1] with a
 * memset on the stream when counts is not NULL.  emit with v_cap == f_cap == 0: returns 0, launches nothing. */
#ifndef CRNERF_MESH_H
#define CRNERF_MESH_H

#include "crnerf.h"

#ifdef __cplusplus
extern "C" {
#endif

size_t crnerf_mesh_workspace_bytes(int32_t nx, int32_t ny, int32_t nz);
int crnerf_mesh_count_f32(const float* sigma, int32_t nx, int32_t ny, int32_t nz, float threshold, void* workspace, int64_t* counts, void* stream);
int crnerf_mesh_emit_f32(const float* sigma, const float* xs, const float* ys, const float* zs, int32_t nx, int32_t ny, int32_t nz, float threshold,
                         const void* workspace, int64_t v_cap, int64_t f_cap, float* vertices, float* normals, int32_t* faces, void* stream);

#ifdef __cplusplus
}
#endif

#endif

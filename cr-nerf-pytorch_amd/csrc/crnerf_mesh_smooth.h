/* STAGED companion header of include/crnerf_mesh_parts.h: Taubin's lambda | mu smoothing of an indexed triangle mesh and area-weighted vertex
 * normals from its faces, on the device -- what takes the noise of a trained density and the blocks of crnerf_mesh_cluster_emit_f32 out of a
 * surface, and gives any mesh normals that belong to its faces, without a copy to the host -- exported from the same libcrnerf_hip.so.  It is
 * staged beside the sources, like crnerf_point_features.h and crnerf_mesh_simplify.h, because the ABI registry is pinned by count
 * (tests/test_host.py: include/ equals the registry's headers), _lib.STAGED_SIGNATURES and _lib.STAGED_MESH_SIGNATURES by their one header each
 * and _lib.STAGED_MAPPINGS by its two mappings (tests/test_mesh_simplify_host.py): _lib.STAGED_SMOOTH_SIGNATURES holds the four rows and load()
 * binds it behind STAGED_MAPPINGS with the same loop.  The follow-up moves the staged files into include/ and their tables into
 * _lib.HEADER_SIGNATURES and edits tests/test_host.py to say so; nothing else about the entries changes.  Conventions (device pointers, `stream`,
 * error codes, crnerf_last_error) are those of crnerf.h; crnerf_abi_version() is unchanged.
 *
 * Input: vertices[V][3] float32 and faces[F][3] int32 -- ANY indexed triangle list; it need not come from crnerf_mesh_emit_f32.
 * Everything below is a function of the input alone: the outputs are the same bytes on every run, whatever order the kernels' atomics happen in,
 * they do not depend on the ORDER of the faces, and a C caller can predict them.
 *
 *   Arithmetic.  Every float64 operation below is rounded on its own: the library is built with -ffp-contract=off and without fast-math, and
 *     the rules rely on it.  rint rounds to nearest, ties to even; integer sums are 64-bit and wrap.
 *   Domain.  Finite coordinates: documented, not checked.  No coordinate is ever used as an index, so a non-finite one never causes an access
 *     outside a buffer; what it does to the positions and normals of its neighbours is unspecified.
 *   Valid faces.  A face is valid iff its three ids lie in [0, V).  An invalid face contributes nothing and is never dereferenced: the kernels
 *     test the ids before they use them (crnerf_mesh_parts.h).
 *   Neighbours.  Each valid face (a, b, c) gives a the neighbours b and c, b the neighbours c and a, c the neighbours a and b.  Multiplicity
 *     counts: an interior edge of a manifold mesh counts twice and a border edge once, a duplicate face counts again.  d_i = the number of
 *     entries of vertex i = 2 x its valid incident faces.
 *   Pinned vertices.  A vertex with d_i = 0 never moves.  With pin_border != 0 a vertex with h_i != 0 never moves either, where
 *     h_i = the sum over its valid incident faces of mix(next) - mix(prev), wrapping in uint64 -- next and prev: the ids that follow and precede
 *     i in the face's cycle --, and mix is the splitmix64 finaliser of the id: z = id + 0x9E3779B97F4A7C15; z = (z ^ (z >> 30)) *
 *     0xBF58476D1CE4E5B9; z = (z ^ (z >> 27)) * 0x94D049BB133111EB; mix = z ^ (z >> 31).  In a consistently oriented manifold mesh the link of
 *     an interior vertex is a closed cycle -- every neighbour is one face's next and another's prev -- so h_i = 0, and at a vertex on an edge
 *     used once the two ends of its open fan remain: exactly the border is pinned.  At a non-manifold vertex this is a stated heuristic; the mix
 *     is there so that two open fans do not cancel by accident of their ids.
 *   Fixed point.  The box is four scalars, lo0, lo1, lo2 (float32, finite) and k (int32 in [-100, 100]):
 *     P_a = clamp(rint(((double) v_a - (double) lo_a) * 2^k), 0, 2^30), an int32.  The clamp is a stated safety: a vertex outside the box
 *     [lo_a, lo_a + 2^(30 - k)] is moved onto it.  crnerf_amd.geometry.Mesh.smooth chooses the box so that the clamp is never met: with E the
 *     largest extent of the bounding box, e = ceil(log2(E)) (E = 0 counts as 1), k = 29 - e and lo_a = float32((min_a + max_a) / 2 - 2^e),
 *     which leaves a margin of at least E / 2 on every side.
 *   One pass with weight w (double).  S_i = the sum of P_j over the neighbour entries of i, exact in int64;
 *     P_i' = clamp((int) rint(Pf + w * ((double) S_i / (double) d_i - Pf)), 0, 2^30) with Pf = (double) P_i: a division, a subtraction, a
 *     product, a sum, rint, in that order, per axis.  A pinned vertex keeps P_i.  Every P_i' is computed from the previous pass's P (Jacobi:
 *     two buffers), so the order of the vertices does not matter either.
 *   One step is a pass with w = lambda followed by a pass with w = mu (Taubin 1995: lambda > 0 smooths, mu < -lambda undoes the shrinkage);
 *     `steps` steps make 2 x steps passes.  mu = 0 is not special: that pass computes Pf + 0 * (...) and changes nothing.
 *   Output.  out_a = (float) ((double) lo_a + ldexp((double) P_a, -k)).  steps = 0 is therefore the quantisation round trip and not a byte copy
 *     of the vertices: a coordinate moves by up to 2^-(k + 1) and one float32 rounding (about 1e-9 on a mesh of unit size).
 *   Exactness domain.  The sums S_i are exact -- below 2^53, so that (double) S_i is S_i -- while a vertex has fewer than 2^21 valid incident
 *     faces.
 *   Face normals per vertex (area-weighted).  For a valid face, in float64: e1 = (double) v_b - (double) v_a, e2 = (double) v_c - (double) v_a,
 *     c = e1 x e2 written out as six products and three differences: c_0 = e1_1 * e2_2 - e1_2 * e2_1, c_1 = e1_2 * e2_0 - e1_0 * e2_2,
 *     c_2 = e1_0 * e2_1 - e1_1 * e2_0.  q_a = (int64) rint(c_a * 2^k2) (clamped to +-2^62 before the conversion), added to each of the
 *     three corners with 64-bit integer adds: N_i.  k2: int32 in [-300, 300]; crnerf_amd.geometry passes k2 = 44 - 2 ceil(log2(E)).
 *     Domain: |q_a| < 2^46 for a mesh inside its box with that k2, so the sums are exact below 2^16 incident faces; beyond, they wrap and are
 *     still deterministic.  Finish: x, y, z = (double) N_i; L = sqrt((x * x + y * y) + z * z); normal = (float) (N_i / L) per axis, and the
 *     zero vector when N_i is zero (a vertex no valid face uses, or faces that cancel).  Faces are counter-clockwise seen from outside
 *     (crnerf_mesh.h), so these normals point the way crnerf_mesh_emit_f32's do.
 *
 * USE: size ONE workspace with crnerf_mesh_smooth_workspace_bytes(V, F); adjacency; then smooth -- as often as wanted: with other vertices,
 * boxes, steps and weights -- with the workspace as adjacency left it and the same V and F.  vertex_normals keeps its sums in a part of the
 * workspace the other two do not touch, and needs no adjacency.  All on one stream.
 *
 * crnerf_mesh_smooth_workspace_bytes: 80 V + 24 F + 8 per 1,024 vertices + 192; 0 for V <= 0 and for sizes the calls refuse.  Every array
 *   inside starts on a 16-byte boundary; the workspace must be 16-byte aligned (CRNERF_ERR_CONFIG otherwise).  The neighbour list, the 24 F, lies
 *   last: a caller that wants vertex_normals alone sizes its workspace with F = 0.
 * crnerf_mesh_adjacency_i32: d_i and h_i by one thread per face with integer atomic adds (equal ids in neighbouring lanes of a wave go out
 *   once); row offsets by a workgroup scan over 1,024 vertices and one single-workgroup pass over the block totals (64-bit); the neighbour
 *   list (6 F entries at most) is filled through a per-vertex cursor.  The order of the entries inside a row differs from run to run: every
 *   sum over a row is an integer sum, so nothing that leaves the library depends on it.  No workgroup waits for another.
 * crnerf_mesh_smooth_f32: one kernel quantises -- P as 16 bytes a vertex, the row's length beside it, 0 for a vertex that stays --, 2 x steps
 *   kernels gather -- no atomics: a thread per vertex, one 16-byte load a neighbour, the lanes of its wave together over a long row --, one
 *   kernel writes out_vertices[V][3] (which may be `vertices`).
 * crnerf_mesh_vertex_normals_f32: one thread per face adds, one thread per vertex finishes into out_normals[V][3].
 *
 * Refusals, on the host before any device work, each with a crnerf_last_error text that starts with "mesh_adjacency: ", "mesh_smooth: " or
 * "mesh_vertex_normals: ": a negative V or F, or one above 2^31 - 1; steps < 0 or steps > 65,536; a lambda or mu that is not finite or has
 * |w| > 2; k outside [-100, 100]; k2 outside [-300, 300]; a lo_a that is not finite (CRNERF_ERR_SHAPE); a NULL pointer with work to do
 * (CRNERF_ERR_NULL); a workspace off 16 bytes (CRNERF_ERR_CONFIG).
 * V == 0: returns 0 and launches nothing.  F == 0 with V > 0 is real work: no vertex has a neighbour, smooth is the round trip and every
 * normal is zero; faces may then be NULL. */
#ifndef CRNERF_MESH_SMOOTH_H
#define CRNERF_MESH_SMOOTH_H

#include "../../include/crnerf.h"   /* "crnerf.h" once this file sits in include/ */

#ifdef __cplusplus
extern "C" {
#endif

size_t crnerf_mesh_smooth_workspace_bytes(int64_t V, int64_t F);
int crnerf_mesh_adjacency_i32(const int32_t* faces, int64_t V, int64_t F, void* workspace, void* stream);
int crnerf_mesh_smooth_f32(const float* vertices, int64_t V, int64_t F, float lo0, float lo1, float lo2, int32_t k, int32_t steps, double lambda,
                           double mu, int32_t pin_border, void* workspace, float* out_vertices, void* stream);
int crnerf_mesh_vertex_normals_f32(const float* vertices, const int32_t* faces, int64_t V, int64_t F, int32_t k2, void* workspace,
                                   float* out_normals, void* stream);

#ifdef __cplusplus
}
#endif

#endif

/* STAGED companion header of include/crnerf_mesh_parts.h: mesh simplification by vertex clustering (Rossignac-Borrel) on the device -- what turns
 * the mesh of crnerf_mesh_emit_f32, whose size follows the sampling grid, into one whose size follows a cell size the caller chooses, without a copy
 * to the host -- exported from the same libcrnerf_hip.so.  It is staged beside the sources, like crnerf_point_features.h, because the ABI registry is
 * pinned by count (tests/test_host.py: include/ equals the registry's headers, 152 rows, nine headers) and _lib.STAGED_SIGNATURES by its one header
 * (tests/test_point_features_host.py): _lib.STAGED_MESH_SIGNATURES holds the three rows and load() binds both staged mappings with one loop.  The
 * follow-up moves both staged files into include/ and their tables into _lib.HEADER_SIGNATURES (157 rows, eleven headers) and edits
 * tests/test_host.py to say so; nothing else about the entries changes.  Conventions (device pointers, `stream`, error codes, crnerf_last_error) are
 * those of crnerf.h; crnerf_abi_version() is unchanged.
 *
 * Input: vertices[V][3] float32 and faces[F][3] int32 -- ANY indexed triangle list; it need not come from crnerf_mesh_emit_f32 --, optionally
 * normals[V][3] and colors[V][3] float32; a grid of n0 x n1 x n2 cells (int32 >= 1, each <= 2^20, n0 n1 n2 <= 2^31 - 1) of size cell0 x cell1 x cell2
 * (float32, finite, > 0, with a finite float32 reciprocal) whose first corner is (lo0, lo1, lo2) (float32, finite).  The grid travels as nine
 * scalars.
 * Everything below is a function of the input alone: the outputs are the same bytes on every run, whatever order the kernels' atomics happen in,
 * and a C caller can predict them.
 *
 *   Arithmetic.  Every float32 and float64 operation below is rounded on its own: the library is built with -ffp-contract=off and without
 *     fast-math, and the rules rely on it.  (int) truncates, floorf and rintf (ties to even) are C's.
 *   Domain.  Finite coordinates, normals and colours: documented, not checked.  The unit is built with -fno-honor-nans, so nothing here is defined
 *     through a comparison with a NaN; a non-finite value never causes an access outside a buffer -- the integers are clamped after every
 *     conversion --, the cell of such a vertex and what it adds to its cluster's sums are unspecified.
 *   Cell of a vertex.  Per axis a: inv_a = 1.0f / cell_a (once, on the host); s_a = (v_a - lo_a) * inv_a, clamped to [0, n_a]: a point outside
 *     the box belongs to the nearest border cell; c_a = min((int) s_a, n_a - 1): a point ON the far face belongs to the last cell.  The cell key is
 *     c0 + n0 * (c1 + n1 * c2).
 *   Clusters.  One cluster per occupied cell.  The leader of a cluster is its smallest member vertex id; the cluster ids 0 .. V'-1 ascend in the
 *     leader's id (the convention of part ids in crnerf_mesh_parts.h).  vertex_cluster[V] int32; counts[0] = V'.
 *   Cluster position.  Exact integer accumulation, so it does not depend on the order of the sums.  Per member and axis:
 *     r_a = (int) floorf((s_a - (float) c_a) * 1048576.0f), in [0, 2^20].  Both operations are exact in float32: (float) c_a is exact (c_a < 2^20);
 *     c_a <= s_a <= c_a + 1 and s_a is a multiple of its own last place, which is no larger than the last place of anything in [0, 1], so the
 *     difference is a multiple of that place no larger than 1 and needs no more digits than s_a had; 1048576 = 2^20 only moves the exponent.
 *     S_a = the sum of r_a over the members, a 64-bit integer (S_a <= 2^31 * 2^20 = 2^51); m = the number of members.
 *     position_a = (float) ((double) lo_a + ((double) c_a + (double) S_a / ((double) m * 1048576.0)) * (double) cell_a).
 *     A vertex ALONE in its cell therefore moves: by less than cell_a * 2^-20 (the floor) plus the roundings of that line -- well under one part
 *     in 10^5 of a cell.  That is why "nothing merged" (cells so small that V' = V) is not a byte copy of the vertices.
 *   Cluster normal (normals given).  Per member q_a = (int) rintf(clamp(normal_a, -1, 1) * 1048576.0f), summed in 64-bit integers to N_a;
 *     d = sqrt((double) N_0 * N_0 + (double) N_1 * N_1 + (double) N_2 * N_2) (three products, two sums, left to right);
 *     normal_a = (float) ((double) N_a / d), and the zero vector when N_0 = N_1 = N_2 = 0.
 *   Cluster colour (colours given).  Per member q_a = (int) rintf(clamp(color_a, 0, 1) * 1048576.0f), summed in 64-bit integers to C_a;
 *     color_a = (float) ((double) C_a / ((double) m * 1048576.0)).
 *   Faces.  A face is valid iff all three ids lie in [0, V).  An invalid face is dropped and never dereferenced: the kernels test the ids
 *     before they use them.  A valid face is mapped to its three cluster ids; it collapses, and is dropped, when two of them are equal.  Of the
 *     surviving faces that name the same SET of three clusters -- whatever their orientation -- only the one with the smallest input index is kept.
 *     Kept faces appear in their input order, each with its cycle as given, rotated so that the smallest id comes first (crnerf_mesh.h,
 *     Rotation).  counts[1] = F'.
 *   Unused clusters.  A cluster no kept face uses stays: it is an unused vertex of the output, which is a part with 0 faces in
 *     crnerf_mesh_parts.h -- selecting the parts with at least one face (crnerf_amd.geometry.Mesh.drop_small(1)) removes it.
 *
 * USE: size ONE workspace with crnerf_mesh_cluster_workspace_bytes(V, F, n0 * n1 * n2); count; read counts[0..1] = V', F' back; allocate; emit
 * with the workspace as count left it, the same vertices, faces and grid, and the vertex_cluster count wrote.  All on one stream.
 *
 * crnerf_mesh_cluster_workspace_bytes: 4 per cell (the dense leader table) + 6 V + 18 F + 4 per slot of a table of the smallest power of two
 *   >= 2 F slots + 84 per possible cluster (min(V, cells)) + 8 per 1,024 vertices + 8 per 1,024 faces + 192; 0 for V <= 0 and for sizes the
 *   calls refuse.  Every array inside starts on a 16-byte boundary; the workspace must be 16-byte aligned (CRNERF_ERR_CONFIG otherwise).
 * crnerf_mesh_cluster_count_f32: the leader table is filled with a sentinel; one pass over the vertices keeps each key and lowers
 *   leader[key] to the vertex id with an atomic minimum (equal keys in neighbouring lanes of a wave go out once); a workgroup scan of the leader
 *   flags and one single-workgroup pass over the block totals (64-bit carry) number the clusters; one pass over the faces maps and sorts their
 *   ids; the survivors are inserted into a lock-free open-addressing table of face indices -- an empty slot is claimed by compare-and-swap, a
 *   slot that holds a face of the same set is lowered with an atomic minimum, any other slot is passed: a slot only ever changes to a face of the
 *   same set, so it ends as the smallest face index of its set whatever order the inserts ran in --; a face is kept iff its slot holds its own
 *   index; a second scan numbers the kept faces.  No workgroup waits for another.  counts[0..1] are written on the device, in stream order.
 * crnerf_mesh_cluster_emit_f32: integer atomic adds on 64-bit words into per-cluster sums (exact: deterministic; equal clusters in neighbouring
 *   lanes of a wave are summed in registers first), one finalising kernel over the clusters, one kernel over the faces.  v_cap / f_cap are the
 *   rows the output buffers hold: a row at or beyond its cap is not written (out_normals and out_colors hold v_cap rows too), so a short buffer
 *   yields a truncated mesh, never a write past it.  normals NULL: out_normals is not touched; colors NULL: out_colors is not touched.
 *
 * Refusals, on the host before any device work, each with a crnerf_last_error text that starts with "mesh_cluster_count: " or
 * "mesh_cluster_emit: ": a negative V, F or capacity, or one above 2^31 - 1; n_a < 1, n_a > 2^20 or n0 n1 n2 > 2^31 - 1; a cell_a that is not
 * finite and > 0 or whose float32 reciprocal is not finite; a lo_a that is not finite (CRNERF_ERR_SHAPE); a NULL pointer with work to do
 * (CRNERF_ERR_NULL); a workspace off 16 bytes (CRNERF_ERR_CONFIG).
 * V == 0: returns 0 and launches nothing; count zeroes counts[0..1] with a memset on the stream when counts is not NULL.  F == 0 with V > 0 is
 * real work: clusters and no faces.  emit with v_cap == 0 and (f_cap == 0 or F == 0): returns 0, launches nothing. */
#ifndef CRNERF_MESH_SIMPLIFY_H
#define CRNERF_MESH_SIMPLIFY_H

#include "../../include/crnerf.h"   /* "crnerf.h" once this file sits in include/ */

#ifdef __cplusplus
extern "C" {
#endif

size_t crnerf_mesh_cluster_workspace_bytes(int64_t V, int64_t F, int64_t cells);
int crnerf_mesh_cluster_count_f32(const float* vertices, const int32_t* faces, int64_t V, int64_t F, float lo0, float lo1, float lo2, float cell0,
                                  float cell1, float cell2, int32_t n0, int32_t n1, int32_t n2, void* workspace, int32_t* vertex_cluster,
                                  int64_t* counts, void* stream);
int crnerf_mesh_cluster_emit_f32(const float* vertices, const float* normals, const float* colors, const int32_t* faces,
                                 const int32_t* vertex_cluster, int64_t V, int64_t F, float lo0, float lo1, float lo2, float cell0, float cell1,
                                 float cell2, int32_t n0, int32_t n1, int32_t n2, void* workspace, int64_t v_cap, int64_t f_cap,
                                 float* out_vertices, float* out_normals, float* out_colors, int32_t* out_faces, void* stream);

#ifdef __cplusplus
}
#endif

#endif

/* Companion header of include/crnerf_mesh.h: the connected parts of an indexed triangle mesh, labelled, measured and filtered on the device --
 * what removes the floaters of a trained density without a copy to the host -- exported from the same libcrnerf_hip.so.  A file of its own because
 * crnerf.h, crnerf_geometry.h and crnerf_mesh.h are pinned, text and prototype count, by the tests of the rounds that wrote them.  Conventions
 * (device pointers, `stream`, error codes, crnerf_last_error) are those of crnerf.h; crnerf_abi_version() is unchanged.
 *
 * Input: faces[F][3] int32 over V vertices -- ANY indexed triangle list; it need not come from crnerf_mesh_emit_f32.
 * Everything below is a function of the input alone: the outputs are the same bytes on every run, whatever order the kernel's unions happen in,
 * and a C caller can predict them.
 *
 *   Valid face.  A face is valid iff all three ids lie in [0, V).  An invalid face joins nothing, gets face_part = -1, is never selected and is
 *     never dereferenced: the kernels test the ids before they use them, so a bad index is not a wild access.
 *   Parts.  Two vertices are connected if some valid face holds both; the parts are the classes of the transitive closure.  A vertex no valid
 *     face uses is a part of its own with 0 faces.  (Connectivity is by shared VERTEX.  For a mesh of crnerf_mesh_emit_f32 this is the same as
 *     connectivity by shared edge: there every vertex's link is one cycle -- or one path, on the border of the grid --, so the faces around a
 *     vertex are joined to one another through edges.)
 *   Part ids.  0 .. K-1, ascending in the smallest vertex id of the part.
 *   Labels.  vertex_part[V] int32; face_part[F] int32 = vertex_part[faces[f][0]] for a valid face, -1 otherwise; counts[0] = K.
 *   Sizes.  part_vertices[K], part_faces[K] int32: how many entries of vertex_part / face_part hold each id.  An entry outside [0, K) is not
 *     counted.
 *   Selection by keep[K] (uint8, non-zero: keep).  An entry of vertex_part / face_part outside [0, K) counts as not kept.
 *     Kept vertices: those whose part is kept, in their original order; the new id is the rank among the kept.  Rows of vertices and normals
 *       are byte copies.
 *     Kept faces: those whose face_part is kept, in their original order, ids replaced by the new ids, the cycle left as it is.  The new ids
 *       rise with the old ones, so "smallest id first" (crnerf_mesh.h, Rotation) survives.
 *     The labels are taken as given.  With labels that do not come from the label call on the same faces, a kept face may name an id outside
 *       [0, V): that id is written as -1 and nothing is dereferenced; or a vertex that is not kept: it gets the rank that vertex would have had.
 *   Largest.  Parts are ranked by part_faces descending, ties to the smaller part id; "the n largest" keeps the first n of that ranking.  This is
 *     a rule for whoever fills keep[] (crnerf_amd.geometry.Mesh.largest does, on the device); the output order is still the original one.
 *
 * USE: size ONE workspace with crnerf_mesh_parts_workspace_bytes(V, F); label (the workspace is scratch, nothing is carried over); read
 * counts[0] = K back; sizes; fill keep[K]; select_count; read counts[0..1] = V', F' back; allocate; select_emit with the workspace as
 * select_count left it and the same labels, K and keep.  All on one stream.
 *
 * crnerf_mesh_parts_workspace_bytes: 6 V + 2 F + 8 per 1,024 vertices + 8 per 1,024 faces + 64; 0 for V <= 0 and for sizes the calls refuse.
 *   The workspace must be 16-byte aligned (CRNERF_ERR_CONFIG otherwise).
 * crnerf_mesh_parts_label_i32: a lock-free union-find over parent[V] in the workspace.  A union always hooks the larger root under the smaller
 *   (one compare-and-swap on the larger root), so the root of a part is its smallest vertex id however the unions interleave; a thread tries
 *   again only when another thread's successful update changed what it had read, and no thread waits for another workgroup.  Then: flatten and
 *   a workgroup scan of the root flags, one single-workgroup pass over the block totals (64-bit carry), apply.  Five launches (four when F = 0).
 * crnerf_mesh_parts_sizes_i32: zeroes both outputs on the stream, then integer atomic adds -- exact, so deterministic --, equal labels summed
 *   inside a wave and then inside a workgroup first: a mesh that is mostly one part costs at most 512 adds to that part's counter, not one
 *   per entry.
 * crnerf_mesh_parts_select_count: workgroup scans of the keep flags, one single-workgroup pass over the block totals; counts[0] = V',
 *   counts[1] = F' are written on the device, in stream order.  vertex_part / face_part may be NULL when V / F is 0.
 * crnerf_mesh_parts_select_emit_f32: v_cap / f_cap are the rows the output buffers hold: a row at or beyond its cap is not written
 *   (out_normals holds v_cap rows too), so a short buffer yields a truncated mesh, never a write past it.  normals NULL: out_normals is not
 *   touched.
 *
 * Refusals, on the host before any device work, each with a crnerf_last_error text that starts with the entry's name less its crnerf_ prefix
 * and type suffix ("mesh_parts_label: ..."): a negative V, F, K or capacity, V, F or a capacity above 2^31 - 1, K > V (CRNERF_ERR_SHAPE); a NULL
 * pointer with work to do (CRNERF_ERR_NULL); a workspace off 16 bytes (CRNERF_ERR_CONFIG).
 * V == 0: returns 0 and launches nothing (face_part is not touched); label and select_count zero their counts with a memset on the stream
 * when counts is not NULL.  F == 0 with V > 0 is real work: V parts of one vertex.  sizes with K == 0 and emit with v_cap == f_cap == 0:
 * return 0, launch nothing. */
#ifndef CRNERF_MESH_PARTS_H
#define CRNERF_MESH_PARTS_H

#include "crnerf.h"

#ifdef __cplusplus
extern "C" {
#endif

size_t crnerf_mesh_parts_workspace_bytes(int64_t V, int64_t F);
int crnerf_mesh_parts_label_i32(const int32_t* faces, int64_t V, int64_t F, void* workspace, int32_t* vertex_part, int32_t* face_part,
                                int64_t* counts, void* stream);
int crnerf_mesh_parts_sizes_i32(const int32_t* vertex_part, const int32_t* face_part, int64_t V, int64_t F, int64_t K, int32_t* part_vertices,
                                int32_t* part_faces, void* stream);
int crnerf_mesh_parts_select_count(const int32_t* vertex_part, const int32_t* face_part, int64_t V, int64_t F, int64_t K, const uint8_t* keep,
                                   void* workspace, int64_t* counts, void* stream);
int crnerf_mesh_parts_select_emit_f32(const float* vertices, const float* normals, const int32_t* faces, const int32_t* vertex_part,
                                      const int32_t* face_part, int64_t V, int64_t F, int64_t K, const uint8_t* keep, const void* workspace,
                                      int64_t v_cap, int64_t f_cap, float* out_vertices, float* out_normals, int32_t* out_faces, void* stream);

#ifdef __cplusplus
}
#endif

#endif

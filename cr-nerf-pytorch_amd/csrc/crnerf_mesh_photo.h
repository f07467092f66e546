/* STAGED companion header of include/crnerf_mesh_parts.h: a z-buffer of an indexed triangle mesh in N posed pinhole views, and per-vertex colours
 * by reprojection of N posed photos -- project every vertex into every photo, drop the views in which it is occluded or faces away, average what
 * the others see -- on the device, without a copy of the mesh to the host; exported from the same libcrnerf_hip.so.  It is staged beside the
 * sources, like crnerf_point_features.h, crnerf_mesh_simplify.h and crnerf_mesh_smooth.h, because the ABI registry is pinned by count
 * (tests/test_host.py: include/ equals the registry's headers), _lib.STAGED_MAPPINGS by its two mappings and _lib.STAGED_SMOOTH_SIGNATURES by
 * its one header: _lib.STAGED_PHOTO_SIGNATURES holds the two rows and load() binds it behind the smooth mapping with the same loop.  The
 * follow-up moves the staged files into include/ and their tables into _lib.HEADER_SIGNATURES and edits tests/test_host.py to say so; nothing
 * else about the entries changes.  Conventions (device pointers, `stream`, error codes, crnerf_last_error) are those of crnerf.h;
 * crnerf_abi_version() is unchanged.
 *
 * Input: vertices[V][3] float32 and faces[F][3] int32 -- ANY indexed triangle list.  Everything below is a function of the input alone: the
 * outputs are the same bytes on every run, whatever order the kernels' atomics happen in, they do not depend on the ORDER of the faces or of
 * the views' visits, and a C caller can predict them.
 *
 *   Arithmetic.  Every float64 operation below is rounded on its own: the library is built with -ffp-contract=off and without fast-math, and
 *     the rules rely on it.  rint rounds to nearest, ties to even.  Every comparison is false on NaN (the unit is built to honour NaNs).
 *   Views.  A view is a pinhole camera in the convention of the training rays (the direction of pixel (i, j) is ((i - cx) / fx, -(j - cy) / fy,
 *     -1) in the camera frame: x right, y up, looking along -z; no half-pixel offset; c2w [3,4]).  Three device arrays describe N views:
 *       cams[N][16]  float64  fx, fy, cx, cy, then R = c2w[:, :3] row-major (9 values), then t = c2w[:, 3] (3 values)
 *       dims[N][2]   int32    (W, H)
 *       offsets[N]   int64    pixel (i, j) of view n is element offsets[n] + j W + i of a flat buffer of total_pixels pixels
 *     The depth buffer is float32, one value a pixel; the photo buffer is 3 uint8 (r, g, b) a pixel with the same indexing.  Views may differ
 *     in size.
 *   Skipped views.  The tables live on the device, so the host cannot check them: the kernels do.  A view is skipped entirely if W < 2 or
 *     H < 2, if W > 16384 or H > 16384, if offsets[n] < 0, or if offsets[n] + W H > total_pixels.  A skipped view is never written and never
 *     counted.  No table entry is ever used as an address before it has passed these tests.  Views that pass may overlap in the buffer; that
 *     is the caller's business (a z-buffer pixel is then the minimum over both).
 *   Projection, the same in both entries, float64, in this order: d_a = (double) x_a - t_a;
 *     cam_k = (d_0 R[0][k] + d_1 R[1][k]) + d_2 R[2][k]; z = -cam_2.  The point is in front of the camera iff z >= z_near: a point with a NaN
 *     coordinate is never in front.  u = cx + fx (cam_0 / z); v = cy - fy (cam_1 / z).  Depth here is this z, the distance along the optical
 *     axis -- NOT the renderer's along-ray depth_fine.  An infinite coordinate either gives a NaN z and is not in front, or a u, v that is NaN
 *     or fails the range tests below, or the camera's centre pixel (cx, cy): no coordinate is ever used as an index before it has been held
 *     to the view's bounds.
 *   Valid faces.  A face is valid iff its three ids lie in [0, V).  An invalid face contributes nothing and is never dereferenced: the kernels
 *     test the ids before they use them (crnerf_mesh_parts.h).
 *
 * crnerf_mesh_zbuffer_f32: depth[total_pixels] is filled with +inf (bits 0x7F800000); every valid face is then rasterised into every view that
 *   is not skipped:
 *   1. Project the three corners.  The face is dropped for this view if a corner is not in front -- there is NO near-plane clipping: a face
 *      that crosses the plane z = z_near is not drawn at all -- or if a |u| or |v| is not below 2^20.
 *   2. Quantise to 4 sub-pixel bits, as int64: X_k = (int64) rint(u_k 16), Y_k = (int64) rint(v_k 16); pixel (i, j) is sampled at (16 i, 16 j).
 *   3. Orientation: orient(a, b, c) = (X_b - X_a)(Y_c - Y_a) - (Y_b - Y_a)(X_c - X_a); A = orient(0, 1, 2).  A == 0: dropped.  A < 0:
 *      corners 1 and 2 are exchanged with their z, and A = -A.  Both orientations are drawn; there is no culling.
 *   4. Pixels: i runs over [max(0, ceil(minX / 16)), min(W - 1, floor(maxX / 16))], j likewise over Y and H.  With P the sample point,
 *      E_0 = orient(1, 2, P), E_1 = orient(2, 0, P), E_2 = orient(0, 1, P): exact integers with E_0 + E_1 + E_2 = A.  The pixel is covered iff
 *      all three are >= 0.  The test is inclusive: under a minimum a pixel on a shared edge may be drawn by both faces, so no fill rule is
 *      needed.
 *   5. Depth at a covered pixel, perspective-correct, float64, in this order: w_k = (double) E_k / (double) A;
 *      iz = (w_0 / z_0 + w_1 / z_1) + w_2 / z_2; D = (float) (1.0 / iz).  It is stored with an unsigned 32-bit atomic minimum on the float's
 *      bits: D is positive (or +inf), so the integer order is the float order.
 *   The result does not depend on the order of the faces, on the order of the atomics, or on how the kernel splits a large bounding box over
 *   lanes.  Kernel: one thread per (face, view) pair, the view the slow grid index; a bounding box of at most 16 pixels is walked by the thread
 *   itself, a larger one by the 64 lanes of its wave together.
 *
 * crnerf_mesh_photo_colors_u8: a view n that is not skipped counts for vertex i iff all of these hold:
 *   1. The vertex is in front.
 *   2. If normals is not NULL and the vertex's normal is not all zero: g = -((n_0 d_0 + n_1 d_1) + n_2 d_2) > 0 with n_a = (double) normal_a
 *      -- the surface faces the camera.
 *   3. 0 <= u <= W - 1 and 0 <= v <= H - 1.
 *   4. If depth is not NULL: z <= (double) D s, where D is the depth at pixel ((int) rint(u), (int) rint(v)) and s = 1.0 + depth_tol, formed
 *      once; +inf passes.
 *   The sample is bilinear in float64: x0 = min((int) floor(u), W - 2), a = u - x0; y0 = min((int) floor(v), H - 2), b = v - y0; per channel,
 *   with p00, p10, p01, p11 the bytes at (x0, y0), (x0 + 1, y0), (x0, y0 + 1), (x0 + 1, y0 + 1) as doubles: top = p00 + a (p10 - p00);
 *   bot = p01 + a (p11 - p01); val = top + b (bot - top); q = (int64) rint(val 65536).
 *   S_c is the int64 sum of q over the counting views and cnt their number.  out_views[i] = cnt (int32);
 *   out_colors[i][c] = (float) ((double) S_c / ((double) cnt 16711680.0)) (16711680 = 255 x 65536: a colour in [0, 1]); zeros when cnt = 0.
 *   The sums are integer sums: the kernel may visit the views in any order.  Kernel: one thread per vertex, looping over the views; a view's
 *   table entries are the same for every lane; no atomics.
 *
 * Refusals, on the host before any device work, each with a crnerf_last_error text that starts with "mesh_zbuffer: " or "mesh_photo_colors: ":
 * a negative V, F or N, or one above 2^31 - 1; total_pixels outside [0, 2^40]; a z_near that is not finite or <= 0; a depth_tol that is not
 * finite or < 0 (CRNERF_ERR_SHAPE); a NULL pointer with work to do (CRNERF_ERR_NULL).
 * Z-buffer: total_pixels == 0 returns 0 and launches nothing (there is no pixel, and every view is skipped); N == 0 or F == 0 with
 * total_pixels > 0 fills the buffer with +inf, and only depth is needed then.  Colours: V == 0 returns 0 and launches nothing; N == 0 with
 * V > 0 writes zeros, and only the outputs are needed then; photos may be NULL when total_pixels == 0 (every view is skipped). */
#ifndef CRNERF_MESH_PHOTO_H
#define CRNERF_MESH_PHOTO_H

#include "../../include/crnerf.h"   /* "crnerf.h" once this file sits in include/ */

#ifdef __cplusplus
extern "C" {
#endif

int crnerf_mesh_zbuffer_f32(const float* vertices, const int32_t* faces, int64_t V, int64_t F, const double* cams, const int32_t* dims,
                            const int64_t* offsets, int64_t N, int64_t total_pixels, double z_near, float* depth, void* stream);
int crnerf_mesh_photo_colors_u8(const float* vertices, const float* normals, int64_t V, const uint8_t* photos, const float* depth,
                                const double* cams, const int32_t* dims, const int64_t* offsets, int64_t N, int64_t total_pixels, double z_near,
                                double depth_tol, float* out_colors, int32_t* out_views, void* stream);

#ifdef __cplusplus
}
#endif

#endif

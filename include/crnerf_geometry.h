/* Companion header of include/crnerf.h: the density query -- sigma of a NeRF_sigma at points that do not come from rays -- exported from the same
 * libcrnerf_hip.so.  It is a file of its own because crnerf.h is pinned, text and prototype count, by the tests of the rounds that wrote it.
 * Conventions (device pointers, `stream`, error codes, crnerf_last_error) are those of crnerf.h; crnerf_abi_version() is unchanged.
 *
 * `packed` is the pack crnerf_mlp_forward_f32 (crnerf_pack_mlp_weights) / crnerf_mlp_forward_bf16 (crnerf_pack_mlp_weights_bf16) take.  What is
 * computed is sigma = static_sigma(xyz_encoding_8(...(PosEmbedding_xyz(point)))), the value column 0 of crnerf_mlp_forward_*(sigma_only = 1) holds
 * for the embedded point -- without the embedded rows: a point costs 12 bytes in and 4 out (the grid: 4 out), the embedding is built in
 * registers, and the weight stream is walked up to the sigma head only (124 of 151 stages on the fp32 core, 992 of 1,208 fragments on the bf16
 * pair core).
 *
 * crnerf_sigma_points_*: xyz[n][3] float32 -> sigma[n].
 * crnerf_sigma_grid_*:   axis arrays xs[nx], ys[ny], zs[nz] (float32, device; any values: non-uniform grids and slabs of a larger grid are fine)
 *   -> sigma[nz][ny][nx]: flat point i has ix = i % nx, iy = (i / nx) % ny, iz = i / (nx * ny) and the coordinates (xs[ix], ys[iy], zs[iz]).
 *
 * _f32: bit-identical to crnerf_posenc_f32(n_freqs = 15) followed by crnerf_mlp_forward_f32(sigma_only = 1) for coordinates with |v| < 64.
 * _bf16: the mixed-precision semantics of crnerf.h "bf16"; the embedding is the fused bf16 renderer's (hardware sin / cos of a two-float argument
 * reduction, rounded to bf16), not the rounded fp32 embedding crnerf_mlp_forward_bf16 is handed.
 * Domain: |coordinate| < 64 (where the stand-alone embedding and the fused one are the same routine; the fused routine degrades beyond 200).
 *
 * Refusals, on the host before any device work: a negative n or axis length, n or nx * ny * nz above 2^31 - 1 (CRNERF_ERR_SHAPE; split the call:
 * slabs of a grid are grids); a NULL pointer with work to do (CRNERF_ERR_NULL).  n == 0 or an axis of length 0: returns 0, nothing is launched. */
#ifndef CRNERF_GEOMETRY_H
#define CRNERF_GEOMETRY_H

#include "crnerf.h"

#ifdef __cplusplus
extern "C" {
#endif

int crnerf_sigma_points_f32(const void* packed, const float* xyz, float* sigma, int64_t n, void* stream);
int crnerf_sigma_points_bf16(const void* packed, const float* xyz, float* sigma, int64_t n, void* stream);
int crnerf_sigma_grid_f32(const void* packed, const float* xs, const float* ys, const float* zs, int32_t nx, int32_t ny, int32_t nz, float* sigma,
                          void* stream);
int crnerf_sigma_grid_bf16(const void* packed, const float* xs, const float* ys, const float* zs, int32_t nx, int32_t ny, int32_t nz, float* sigma,
                           void* stream);

#ifdef __cplusplus
}
#endif

#endif

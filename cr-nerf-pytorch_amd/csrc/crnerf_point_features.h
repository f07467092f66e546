/* STAGED companion header of include/crnerf.h: the point-feature query -- the 64 rgb features (and sigma) of a NeRF_sigma at points that do not
 * come from rays, each seen from a direction of its own -- exported from the same libcrnerf_hip.so.  It is staged beside the sources because the
 * ABI registry is pinned by count (tests/test_host.py: include/ equals the registry's headers, 152 rows, nine headers, nine held-back symbols):
 * _lib.STAGED_SIGNATURES binds the two rows behind the registry loop.  The follow-up moves this file into include/ and its table into
 * _lib.HEADER_SIGNATURES, counts it there (154 rows, ten headers) and edits tests/test_host.py to say so; nothing else about the entries changes.
 * Conventions (device pointers, `stream`, error codes, crnerf_last_error) are those of crnerf.h; crnerf_abi_version() is unchanged.
 *
 * `packed` is the pack crnerf_mlp_forward_f32 (crnerf_pack_mlp_weights) / crnerf_mlp_forward_bf16 (crnerf_pack_mlp_weights_bf16) take.  What is
 * computed is the module's forward at the embedded point and direction: feature = static_rgb(dir_encoding(cat[xyz_encoding_final(h8),
 * PosEmbedding_dir(dir)])) and sigma = static_sigma(h8), h8 = xyz_encoding_8(...(PosEmbedding_xyz(point))) -- columns 0..63 and 64 of
 * crnerf_mlp_forward_*(sigma_only = 0) on the row cat[posenc(point, 15), posenc(dir, 4)] -- without the embedded rows: a point costs 24 bytes in and
 * 256 (+ 4) out, both embeddings are built in registers, and every tile walks the whole weight stream.
 *
 * crnerf_feature_points_*: xyz[n][3], dirs[n][3] float32 -> feature[n][64] float32, rows 64 wide, pixel-major: the content
 *   crnerf_crossray_decode_f32 reads in place (HW = n).  sigma[n] is filled too unless sigma is NULL.
 *   dirs are taken as given (not normalised); a zero direction is defined: its embedding is sin 0 / cos 0 at every frequency.
 *
 * _f32: bit-identical to crnerf_posenc_f32(xyz, 15), crnerf_posenc_f32(dirs, 4), a cat into [n][120] rows and crnerf_mlp_forward_f32(sigma_only = 0)
 *   for coordinates and direction components with |v| < 64.
 * _bf16: the mixed-precision semantics of crnerf.h "bf16"; both embeddings are the fused bf16 renderer's (hardware sin / cos of a two-float argument
 *   reduction, rounded to bf16), not the rounded fp32 embedding crnerf_mlp_forward_bf16 is handed.
 * Domain: |coordinate| < 64 and |direction component| < 64, as in crnerf_geometry.h (where the stand-alone embedding and the fused one are the same
 *   routine; the fused routine degrades beyond 200).
 * Points are indexed with 32 bits: n <= 2^31 - 1 in one call (split the list).  No load runs past xyz + 3n or dirs + 3n, no store past
 *   feature + 64n or sigma + n.
 *
 * Refusals, on the host before any device work: a negative n, n above 2^31 - 1 (CRNERF_ERR_SHAPE; split the call); a NULL packed, xyz, dirs or
 * feature with n > 0 (CRNERF_ERR_NULL, the message names the field).  n == 0: returns 0, nothing is launched, no pointer is looked at. */
#ifndef CRNERF_POINT_FEATURES_H
#define CRNERF_POINT_FEATURES_H

#include "../../include/crnerf.h"   /* "crnerf.h" once this file sits in include/ */

#ifdef __cplusplus
extern "C" {
#endif

int crnerf_feature_points_f32(const void* packed, const float* xyz, const float* dirs, float* feature, float* sigma, int64_t n, void* stream);
int crnerf_feature_points_bf16(const void* packed, const float* xyz, const float* dirs, float* feature, float* sigma, int64_t n, void* stream);

#ifdef __cplusplus
}
#endif

#endif

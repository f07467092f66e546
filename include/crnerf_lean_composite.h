/* Second companion header of include/crnerf.h, included by crnerf_lean.h: the two launches behind lean=True in the composite precisions "bf16_hc"
 * and "bf16_fc" (a coarse pass on an fp32-accurate or fp16 core, the fine pass on the bf16 pair core), exported from the same libcrnerf_hip.so.
 * It is a file of its own only because tests/test_lean_pair_host.py pins the text of crnerf_lean.h to its two prototypes; folding the headers is
 * moving these declarations behind crnerf_render_rays_lean_f16.  Conventions (device pointers, `stream`, error codes, crnerf_last_error) are
 * those of crnerf.h; every entry takes crnerf_render_args; crnerf_abi_version() is unchanged.
 *
 * crnerf_render_coarse_weights_f32h2 / _f32x3 / _f16: the coarse-only render (n_importance == 0) of crnerf_render_rays_f32h2 / _f32x3 / _f16 for a
 * caller that reads weights_coarse alone -- what sample_pdf needs.  Same packs as those entries.  Every 32-point tile stops behind xyz_encoding_8 /
 * static_sigma: 1,984 of 2,416 weight fragments on the h2 core, 2,976 of 3,648 on the x3 core, 992 of 1,208 on the pair core.  Alpha, the
 * transmittance scan and weights_coarse [n_rays, n_samples] are the full kernel's, BIT-IDENTICAL to its weights_coarse on the same arguments
 * (tests/test_gpu_lean_composite.py); no feature or depth sum is formed and nothing else is stored.
 *   Requires n_importance == 0 and n_samples in [2,256] (CRNERF_ERR_SHAPE); packed_coarse, rays and weights_coarse (CRNERF_ERR_NULL).
 * feature_coarse, depth_coarse, packed_fine, u, noise_fine and every fine pointer are ignored (may be NULL).  z_coarse, z_steps, noise_coarse,
 * noise_std and use_disp as in the full entries; view_dir is accepted and does not matter (the trunk does not read the direction).
 * rng_flags != 0 or any *_out pointer returns CRNERF_ERR_CONFIG.
 *   The mark (_f32h2, _f16).  The full kernels mark a ray with a point that left fp16's range by a NaN feature_coarse row.  There is no such row
 * here, so the mark is the word 0x7fc00000 in weights_coarse[r][0]; the rest of a marked row is unspecified.  A ray is marked when the xyz
 * embedding or an operand of layers 1..8 of one of its points left fp16's range (_f16: or the output of layer 8, which that core converts too),
 * and every ray is marked when the pack carries the range flag.  The full kernels' mark also covers xyz_encoding_final, dir_encoding, static_rgb and
 * the direction embedding, which this walk does not evaluate and whose overflow does not reach the weights: a ray that overflows there only is
 * repaired by the full path (crnerf_render_rays_f32x3_repair) and not by this one.
 *   crnerf_render_coarse_weights_f32x3_repair: the same arguments with the x3 pack of the coarse model.  One workgroup per ray quad; it leaves at
 * once unless weights_coarse[r][0] of one of the quad's four rays holds the mark (a bit test), otherwise it renders the quad's four rows again on
 * the x3 core -- rows that then equal crnerf_render_coarse_weights_f32x3's.  n_rays < 2^33.
 *
 * crnerf_render_rays_lean_bf16_fine: crnerf_render_rays_bf16_fine without weights_fine.  weights_coarse is the INPUT [n_rays, n_samples];
 * sample_pdf, the z merge and the fine model on the bf16 pair core in one launch.  Requires n_importance in [1,256], n_samples in [3,256]
 * (CRNERF_ERR_SHAPE), packed_fine, rays, weights_coarse, feature_fine and depth_fine; weights_fine is ignored (may be NULL), z_fine is optional.
 * feature_fine, depth_fine and z_fine are BIT-IDENTICAL to crnerf_render_rays_bf16_fine's. */
#ifndef CRNERF_LEAN_COMPOSITE_H
#define CRNERF_LEAN_COMPOSITE_H

#include "crnerf.h"

#ifdef __cplusplus
extern "C" {
#endif

int crnerf_render_coarse_weights_f32h2(const crnerf_render_args* args, void* stream);
int crnerf_render_coarse_weights_f32x3(const crnerf_render_args* args, void* stream);
int crnerf_render_coarse_weights_f32x3_repair(const crnerf_render_args* args, void* stream);
int crnerf_render_coarse_weights_f16(const crnerf_render_args* args, void* stream);
int crnerf_render_rays_lean_bf16_fine(const crnerf_render_args* args, void* stream);

#ifdef __cplusplus
}
#endif

#endif

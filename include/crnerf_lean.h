/* Companion header of include/crnerf.h: the lean inference render (crnerf.h "Lean inference render", crnerf_render_rays_lean_f32) on the pair
 * core's two builds, exported from the same libcrnerf_hip.so.  It lives beside crnerf.h only so that crnerf.h and what pins it stay byte for
 * byte as they were; folding the two is moving these declarations behind crnerf_render_rays_lean_f32.  Conventions (device pointers, `stream`,
 * error codes, crnerf_last_error) are those of crnerf.h; crnerf_abi_version() is unchanged.
 *
 * crnerf_render_rays_lean_bf16 / _f16 are crnerf_render_rays_bf16 / crnerf_render_rays_f16 for a caller that reads only the fine image: same
 * struct, same packs (crnerf_pack_mlp_weights_bf16 / _f16), same mixed-precision semantics.  The coarse pass is evaluated for its compositing
 * weights alone, so its 32-point tiles stop behind xyz_encoding_8 / static_sigma (992 of the 1,208 fragments of the weight stream), no coarse
 * feature is composited, and neither the coarse outputs nor weights_fine go to HBM.
 *   Requires n_importance in [1,256], n_samples in [3,256] (CRNERF_ERR_SHAPE) and packed_fine.  weights_coarse, feature_coarse, depth_coarse and
 * weights_fine are ignored (may be NULL); feature_fine and depth_fine are required, z_fine is optional.  z_coarse, z_steps, u / u_stride,
 * noise_coarse / noise_fine, noise_std, view_dir and use_disp as in crnerf_render_rays_bf16.  rng_flags != 0 or any *_out pointer returns
 * CRNERF_ERR_CONFIG (the pair core draws nothing in the kernel).
 *   feature_fine, depth_fine and z_fine are BIT-IDENTICAL to the full entry point's on the same arguments (tests/test_gpu_lean_pair.py).
 *   _f16, range guard: the full kernel marks a ray whose coarse pass left fp16's range with a NaN feature_coarse row and goes on to return finite
 * fine numbers sampled from a wrong pdf.  The lean kernel has no feature_coarse: a ray with a coarse point whose xyz embedding or whose output of
 * one of layers 1..8 left fp16's range returns ALL 64 values of its feature_fine row and its depth_fine as NaN; every other ray is bit-identical
 * to crnerf_render_rays_f16's.  (The full kernel's mark also covers xyz_encoding_final, dir_encoding and the direction embedding of the coarse
 * pass, which the lean kernel does not evaluate and whose overflow does not reach its weights.)  A pack that carries the range flag marks
 * feature_fine[r][0] of every ray, as crnerf_render_rays_f16 does, and writes nothing else. */
#ifndef CRNERF_LEAN_H
#define CRNERF_LEAN_H

#include "crnerf.h"
#include "crnerf_lean_composite.h"   /* the coarse-weights renders and the lean fine launch behind lean=True in "bf16_hc" / "bf16_fc" */

#ifdef __cplusplus
extern "C" {
#endif

int crnerf_render_rays_lean_bf16(const crnerf_render_args* args, void* stream);
int crnerf_render_rays_lean_f16(const crnerf_render_args* args, void* stream);

#ifdef __cplusplus
}
#endif

#endif

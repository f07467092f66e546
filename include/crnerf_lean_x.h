/* Third companion header of include/crnerf.h: the lean inference render (crnerf.h "Lean inference render", crnerf_render_rays_lean_f32;
 * crnerf_lean.h for the pair core) on the two fp32-accurate split cores -- what precision "f32x3", "f32h2" and "auto" run on -- exported from
 * the same libcrnerf_hip.so.  It is a file of its own only because crnerf.h, crnerf_lean.h and crnerf_lean_composite.h are pinned, text and
 * prototype count, by the tests of the rounds that wrote them; folding the headers is moving these declarations behind
 * crnerf_render_rays_lean_f16.  Conventions (device pointers, `stream`, error codes, crnerf_last_error) are those of crnerf.h; every entry
 * takes crnerf_render_args; crnerf_abi_version() is unchanged.
 *
 * crnerf_render_rays_lean_f32x3 / _f32h2 are crnerf_render_rays_f32x3 / _f32h2 for a caller that reads only the fine image: same struct, same
 * packs (crnerf_pack_mlp_weights_x3 / _h2).  The coarse pass is evaluated for its compositing weights alone, so its 32-point tiles stop behind
 * xyz_encoding_8 / static_sigma (2,976 of the 3,648 weight fragments on the x3 core, 1,984 of 2,416 on the h2 core; the weight ring fetches the
 * shorter walk for coarse tiles and the whole stream for fine ones within one launch), no coarse feature or depth is composited, and neither the
 * coarse outputs nor weights_fine go to HBM.
 *   Requires n_importance in [1,256], n_samples in [3,256] (CRNERF_ERR_SHAPE); packed_coarse, packed_fine, rays, feature_fine and depth_fine
 * (CRNERF_ERR_NULL).  weights_coarse, feature_coarse, depth_coarse and weights_fine are ignored (may be NULL) and never touched; z_fine is
 * optional.  z_coarse, z_steps, u / u_stride, noise_coarse / noise_fine, noise_std, view_dir and use_disp as in the full entries.
 * rng_flags != 0 or any *_out pointer returns CRNERF_ERR_CONFIG (there is no lean kernel with in-kernel draws: hand them over as tensors).
 *   feature_fine, depth_fine and z_fine are BIT-IDENTICAL to the full entry's on the same arguments (tests/test_gpu_lean_x.py).
 *   The mark (_f32h2).  The full kernel marks a ray whose coarse pass left fp16's range with a NaN feature_coarse row and goes on to return finite
 * fine numbers sampled from a wrong pdf.  There is no coarse row here: a ray with a coarse point whose xyz embedding or an operand of layers 1..8
 * left fp16's range returns ALL 64 values of its feature_fine row and its depth_fine as NaN.  A fine point that leaves the range poisons
 * feature_fine as in the full kernel; every other ray is bit-identical to crnerf_render_rays_f32h2's.  (The full kernel's coarse mark also covers
 * xyz_encoding_final, dir_encoding, static_rgb and the direction embedding of the coarse pass, which this walk does not evaluate and whose overflow
 * does not reach the weights.)  A pack that carries the range flag marks feature_fine[r][0] of every ray and renders nothing.
 *   crnerf_render_rays_lean_f32x3_repair: the same arguments with the x3 packs.  One workgroup per ray quad; it leaves at once unless
 * feature_fine[r][0] of one of the quad's four rays is a NaN (a bit test; no other buffer is read), otherwise it renders the quad's four rays
 * again, lean, on the x3 core -- rows that then equal crnerf_render_rays_lean_f32x3's.  n_rays < 2^33.  _f32h2 followed by _f32x3_repair on the
 * same block is what precision "auto" with lean=True launches. */
#ifndef CRNERF_LEAN_X_H
#define CRNERF_LEAN_X_H

#include "crnerf.h"

#ifdef __cplusplus
extern "C" {
#endif

int crnerf_render_rays_lean_f32x3(const crnerf_render_args* args, void* stream);
int crnerf_render_rays_lean_f32h2(const crnerf_render_args* args, void* stream);
int crnerf_render_rays_lean_f32x3_repair(const crnerf_render_args* args, void* stream);

#ifdef __cplusplus
}
#endif

#endif

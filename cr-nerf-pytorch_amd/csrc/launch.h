// The launch layer between abi.hip and the kernels, host code only: what every render / MLP launcher did by hand -- the persistent grid plan, the
// launch itself, the renderers' shared argument checks, the fill of a kernel's parameter block from a RenderArgs and the training twin's saved-state
// preparation.  Device code and the kernel parameter blocks (RenderParams16 / X / P, their fields and field order) stay per core: kernarg offsets
// are ISA.  Nothing here allocates or formats on the success path; an error text is composed only once its check has failed (abi.hip fail()).
#pragma once
#include "kernels.h"

namespace crnerf {

// Persistent grid: one workgroup per CU walking `units` (ray quads, point groups) in `iters` rounds; one_per_unit (the repair launches): a
// workgroup per unit, which leaves at once unless its unit needs the work.  units > 0, and <= INT_MAX when one_per_unit.
struct GridPlan { int grid, iters; };
inline GridPlan plan_grid(long units, bool one_per_unit = false) {
  const int cus = num_cus();
  const int grid = one_per_unit ? (int)units : (int)(units < cus ? units : cus);
  return {grid, (int)((units + grid - 1) / grid)};
}

// `what` is the name an error is reported under: the rng instantiations report under the plain kernel's
template <class... P, class... A>
inline int launch_kernel(void (*kernel)(P...), const char* what, int grid, int block, size_t lds_bytes, hipStream_t stream, const A&... args) {
  if (int rc = ensure_dynamic_lds((const void*)kernel, lds_bytes, what)) return rc;
  hipLaunchKernelGGL(kernel, dim3(grid), dim3(block), lds_bytes, stream, args...);
  return check_launch(what);
}

// the sample counts every fused renderer is built for; max_nc, max_ni: the core's MAX_NC, MAX_NI (ray_ops.h, device code: not included here)
inline int check_sample_counts(const char* who, const RenderArgs& a, int max_nc, int max_ni) {
  if (a.Nc < 2 || a.Nc > max_nc) return launch_fail(-2, who, "N_samples must be in [2, 256] for the fused kernel");
  if (a.Ni < 0 || a.Ni > max_ni) return launch_fail(-2, who, "N_importance must be in [0, 256] for the fused kernel");
  if (a.Ni > 0 && a.Nc < 3) return launch_fail(-2, who, "hierarchical sampling needs N_samples >= 3");
  if (a.Ni > 0 && !a.packed_fine) return launch_fail(-3, who, "N_importance > 0 but no fine model");
  return 0;
}

// the fields every kernel parameter block has (iters, sched and a core's own fields are the launcher's)
template <class K>
inline void fill_render_params(K& k, const RenderArgs& a) {
  k.packed0 = (const char*)a.packed_coarse;
  k.packed1 = (const char*)(a.packed_fine ? a.packed_fine : a.packed_coarse);
  k.rays = a.rays; k.view_dir = a.view_dir; k.z_coarse = a.z_coarse; k.z_steps = a.z_steps; k.u = a.u; k.u_stride = a.u_stride;
  k.noise_c = a.noise_coarse; k.noise_f = a.noise_fine; k.noise_std = a.noise_std; k.use_disp = a.use_disp;
  k.R = a.R; k.Nc = a.Nc; k.Ni = a.Ni;
  k.weights_c = a.weights_coarse; k.feature_c = a.feature_coarse; k.depth_c = a.depth_coarse;
  k.weights_f = a.weights_fine; k.feature_f = a.feature_fine; k.depth_f = a.depth_fine; k.z_fine = a.z_fine;
}
// the in-kernel draws (the cores that have them)
template <class K>
inline void fill_rng_params(K& k, const RenderArgs& a) {
  k.rng_seed = a.rng_seed; k.rng_ray_offset = a.rng_ray_offset; k.rng_flags = a.rng_flags; k.perturb = a.perturb;
  k.z_coarse_out = a.z_coarse_out; k.noise_c_out = a.noise_coarse_out; k.noise_f_out = a.noise_fine_out;
}
// the instantiation with the draws also writes z_coarse_out without drawing anything
inline bool wants_rng_kernel(const RenderArgs& a) { return a.rng_flags != 0 || a.z_coarse_out; }

// the training twin's saved state is all there
inline int check_train_state(const char* who, const RenderArgs& a) {
  if (a.Ni > 0 && (!a.train_acts_fine || !a.train_raw_fine)) return launch_fail(-1, who, "fine buffers are NULL");
  if (!a.train_raw_coarse) return launch_fail(-1, who, "raw_coarse is NULL");
  return 0;
}
// the range words of both passes start at zero (kernels.h acts_range_word)
inline int zero_train_ranges(const RenderArgs& a, hipStream_t stream) {
  if (int rc = zero_acts_range(a.train_acts_coarse, a.R * a.Nc, stream)) return rc;
  return a.Ni > 0 ? zero_acts_range(a.train_acts_fine, a.R * (a.Nc + a.Ni), stream) : 0;
}

}  // namespace crnerf

// The lean render on the h2 core (crnerf_render_rays_lean_f32h2, include/crnerf_lean_x.h): render_fused_h2.hip's LEAN body as a unit of its own --
// render_rays_lean_h2_kernel and its launch, nothing else -- so that the unit of the other five kernels compiles as it did without it.
#define CRNERF_X_LEAN_UNIT
#include "render_fused_h2.hip"

// The lean render on the x3 core (crnerf_render_rays_lean_f32x3 / _f32x3_repair, include/crnerf_lean_x.h): render_fused_x3.hip's LEAN body as a unit of
// its own -- render_rays_lean_x3_kernel and its launch, nothing else -- so that the unit of the other five kernels compiles as it did without it.
#define CRNERF_X_LEAN_UNIT
#include "render_fused_x3.hip"

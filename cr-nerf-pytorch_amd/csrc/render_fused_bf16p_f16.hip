// Fused volumetric renderer with one-piece FP16 operands (crnerf_render_rays_f16; include/crnerf.h "f16"): render_fused_bf16p.hip's inference kernel
// built on the fp16 form of the pair core (mlp_core_bf16.h CRNERF_P_F16: v_mfma_f32_32x32x16_f16, v_cvt_pk_f16_f32, range guard).  A ray with a
// point whose operands left fp16's range comes out with a NaN feature row -- what crnerf_render_rays_f32x3_repair re-renders.  Packs from
// crnerf_pack_mlp_weights_f16.
#define CRNERF_P_F16 1
#define CRNERF_P_RENDER_KERNEL render_rays_f16p_kernel
#define CRNERF_P_RENDER_LEAN_KERNEL render_rays_f16p_lean_kernel
#define CRNERF_P_RENDER_LEAN_NAME "render_rays_f16p_lean_kernel"
#define CRNERF_P_RENDER_LAUNCH launch_render_rays_f16p
#define CRNERF_P_RENDER_SCHED crnerf_sched_f16p
#define CRNERF_P_RENDER_NAME "render_rays_f16p_kernel"
#define CRNERF_P_RENDER_WHAT "render_rays_f16"
#include "render_fused_bf16p.hip"

// Stand-alone NeRF_sigma forward with one-piece FP16 operands (crnerf_mlp_forward_f16; include/crnerf.h "f16"): mlp_forward_bf16p.hip built on the
// fp16 form of the pair core (mlp_core_bf16.h CRNERF_P_F16: v_mfma_f32_32x32x16_f16, v_cvt_pk_f16_f32, range guard).  Packs from
// crnerf_pack_mlp_weights_f16.
#define CRNERF_P_F16 1
#define CRNERF_P_MLP_KERNEL mlp_forward_f16p_kernel
#define CRNERF_P_MLP_LAUNCH launch_mlp_forward_f16p
#define CRNERF_P_MLP_NAME "mlp_forward_f16p_kernel"
#include "mlp_forward_bf16p.hip"

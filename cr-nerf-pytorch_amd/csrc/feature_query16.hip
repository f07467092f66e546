// Point-feature query on the v16 core (mlp_core16.h): the 64 rgb features (and sigma) of NeRF_sigma at points that do not come from rays -- a
// point list xyz[n][3] with a view direction dirs[n][3] each (crnerf_point_features.h).  The full-walk twin of the density query
// (sigma_query16.hip): the composed route (crnerf_posenc_f32 twice, a cat into [n,120] rows, crnerf_mlp_forward_f32) moves ~2.1 kB per point
// through HBM; here 24 bytes are read and 256 (+4) leave.  Both embeddings are built in registers (posenc_regs16); the direction differs per
// point, so it stays in registers as in the module entry (DirRegs, mlp_forward16.hip), not parked in LDS as the renderer parks a ray's.  Every
// tile is a full walk (WeightPipe16Infer: all 151 stages).
// The arithmetic is the composed route's: posenc_regs16 is the routine pack.hip's posenc uses below |v| = 64 and mlp_tile16 is the module
// entry's tile -- feature and sigma are bit-identical to it there (tests/test_gpu_point_features.py).
// feature rows are 64 wide, pixel-major: what crnerf_crossray_decode_f32 reads in place.
// Schedule levers (mlp_core16.h): both taken as the inference kernels ship them (CRNERF_CORE16_LAG, CRNERF_CORE16_PRIO).
#include <hip/hip_runtime.h>
#include "kernels.h"
#include "launch.h"
#include "mlp_core16.h"

namespace crnerf {

__global__ __launch_bounds__(512, 2) void feature_points16_kernel(const char* __restrict__ packed, const float* __restrict__ xyz,
                                                                  const float* __restrict__ dirs, float* __restrict__ feature,
                                                                  float* __restrict__ sigma_out, uint32_t n, int iters) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  lds_char* lds = (lds_char*)smem;
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int p = lane & 15, g = lane >> 4;

  load_consts(lds, packed, packed);
  WeightPipe16Infer pipe;
  pipe.start(lds, packed + CONST_BYTES, packed + CONST_BYTES, 1, 1, lane, wave);
  f32x4 q[V16_AHEAD];
  pipe.prime(q);
  PhaseTimer tm;
  tm.start(false);

#pragma unroll 1
  for (int it = 0; it < iters; ++it) {
    // < n + 128 * gridDim.x <= 2^31 + 2^15: unsigned 32-bit holds it (all eight waves walk, also when their tile is past the end)
    const uint32_t i = (((uint32_t)it * gridDim.x + blockIdx.x) * V16_WAVES + wave) * 16u + p;
    const bool valid = i < n;
    // a lane past the end reads row 0: no load beyond xyz + 3n or dirs + 3n; the row offset is formed in 64 bits
    const size_t row = (size_t)(valid ? i : 0u) * 3;
    const float x = xyz[row], y = xyz[row + 1], z = xyz[row + 2];
    const float dx = dirs[row], dy = dirs[row + 1], dz = dirs[row + 2];
    f32x4 pe[6], feat[4];
    DirRegs dreg;
    posenc_regs16<XYZ_FREQS, 6>(x, y, z, g, pe);
    posenc_regs16<DIR_FREQS, 2>(dx, dy, dz, g, dreg.v);
    float sigma;
    mlp_tile16(pipe, 0, pe, dreg, feat, sigma, g, q, tm);
    if (valid) {
      float* o = feature + (size_t)i * FEAT_DIM;
#pragma unroll
      for (int T = 0; T < 4; ++T)
#pragma unroll
        for (int r = 0; r < 4; ++r) o[16 * T + 4 * g + r] = feat[T][r];
      if (sigma_out && g == 0) sigma_out[i] = sigma;
    }
  }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
}

// n in [1, 2^31 - 1], no NULL but sigma (abi.hip has checked)
int launch_feature_points16(const void* packed, const float* xyz, const float* dirs, float* feature, float* sigma, long n, hipStream_t stream) {
  const GridPlan plan = plan_grid((n + 127) / 128);   // 128 points per workgroup-iteration (8 waves x 16)
  return launch_kernel(feature_points16_kernel, "feature_points16_kernel", plan.grid, 512, LDS_SCRATCH, stream, (const char*)packed, xyz, dirs, feature, sigma,
                       (uint32_t)n, plan.iters);
}

}  // namespace crnerf

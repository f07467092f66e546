// Point-feature query on the bf16 pair core (mlp_core_bf16p.h): the 64 rgb features (and sigma) of NeRF_sigma at points that do not come from
// rays -- a point list xyz[n][3] with a view direction dirs[n][3] each (crnerf_point_features.h), in the mixed-precision semantics of
// include/crnerf.h "bf16".  The full-walk twin of the density query (sigma_query_bf16p.hip): 24 bytes per point are read, both embeddings are
// built in registers as the fused renderer builds them (posenc_b), the direction's is stored to the lane's own 64-byte LDS slot exactly as the
// module entry parks a gathered one (mlp_forward_bf16p.hip: it differs per point), every 32-point tile is a full walk (PFullWalk: all 1,208
// fragments) and 256 (+4) bytes per point leave.  No embedded row in HBM.
// No ring-phase toggle (sigma_query_bf16p.hip keeps one): a full walk is whole turns of the four-slot ring.  All eight waves walk every
// iteration, also when their tile is past the end: the ring's barriers need identical control flow.
// feature rows are 64 wide, pixel-major: what crnerf_crossray_decode_f32 reads in place.
#include <hip/hip_runtime.h>
#include "kernels.h"
#include "launch.h"
#include "mlp_core_bf16p.h"

namespace crnerf {

constexpr int LDS_DIR_Q = LDS_SCRATCH_P;                    // 8 waves x 64 lanes x 64 B: every POINT's direction embedding as B operands (dword 32 s)
constexpr int LDS_TOTAL_Q = LDS_DIR_Q + P_WAVES * 64 * 64;  // = mlp_forward_bf16p.hip's LDS_TOTAL_M
static_assert(LDS_TOTAL_Q <= 160 * 1024, "LDS budget");
static_assert(KS_DIR * 32 <= 64, "a lane's slot holds its direction embedding");

__global__ __launch_bounds__(512, 2) void feature_points_bf16p_kernel(const char* __restrict__ packed, const float* __restrict__ xyz,
                                                                      const float* __restrict__ dirs, float* __restrict__ feature,
                                                                      float* __restrict__ sigma_out, uint32_t n, int iters) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  lds_char* lds = (lds_char*)smem;
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int p = lane & 31, h = lane >> 5;

  load_consts(lds, packed, packed);
  lds_char* dirbuf = lds + LDS_DIR_Q + wave * (64 * 64) + lane * 64;   // this lane's own 2 x 16 bytes
  WeightPipeP pipe;
  pipe.start(lds, packed + CONST_BYTES, packed + CONST_BYTES, 0, lane, wave);
  u32x4 q[B_AHEAD];
  pipe.prime(q);
  PhaseTimer tm;
  tm.start(false);
  NoSaveP sv;

#pragma unroll 1
  for (int it = 0; it < iters; ++it) {
    // < n + 256 * gridDim.x <= 2^31 + 2^16: unsigned 32-bit holds it
    const uint32_t i = (((uint32_t)it * gridDim.x + blockIdx.x) * P_WAVES + wave) * 32u + p;
    const bool valid = i < n;
    // a lane past the end reads row 0: no load beyond xyz + 3n or dirs + 3n; the row offset is formed in 64 bits
    const size_t row = (size_t)(valid ? i : 0u) * 3;
    const float x = xyz[row], y = xyz[row + 1], z = xyz[row + 2];
    const float dx = dirs[row], dy = dirs[row + 1], dz = dirs[row + 2];
    u32x4 pe[KS_XYZ], dv[KS_DIR];
    posenc_b<XYZ_FREQS, KS_XYZ>(x, y, z, h, pe);
    posenc_b<DIR_FREQS, KS_DIR>(dx, dy, dz, h, dv);
#pragma unroll
    for (int s = 0; s < KS_DIR; ++s) *(__attribute__((address_space(3))) u32x4*)(dirbuf + 32 * s) = dv[s];
    f32x16 feat[2];
    float sigma;
    mlp_tile_p(pipe, 0, 0, pe, dirbuf, feat, sigma, h, q, tm, sv);   // (reads its lane's dirbuf after its own writes: same wave, in order)
    if (valid) {
      float* o = feature + (size_t)i * FEAT_DIM;
#pragma unroll
      for (int t = 0; t < 2; ++t)
#pragma unroll
        for (int r = 0; r < 16; ++r) o[32 * t + 8 * (r >> 2) + 4 * h + (r & 3)] = feat[t][r];
      if (sigma_out && h == 0) sigma_out[i] = sigma;
    }
  }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
}

// n in [1, 2^31 - 1], no NULL but sigma (abi.hip has checked)
int launch_feature_points_bf16p(const void* packed, const float* xyz, const float* dirs, float* feature, float* sigma, long n, hipStream_t stream) {
  const GridPlan plan = plan_grid((n + 255) / 256);   // 256 points per workgroup-iteration (eight 32-point tiles)
  return launch_kernel(feature_points_bf16p_kernel, "feature_points_bf16p_kernel", plan.grid, 512, LDS_TOTAL_Q, stream, (const char*)packed, xyz, dirs, feature,
                       sigma, (uint32_t)n, plan.iters);
}

}  // namespace crnerf

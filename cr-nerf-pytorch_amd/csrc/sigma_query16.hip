// Density query on the v16 core (mlp_core16.h): sigma of NeRF_sigma at points that do not come from rays -- a point list xyz[n][3], or the
// nodes of a grid given by three axis arrays (include/crnerf_geometry.h).  The stand-alone forward (mlp_forward16.hip, sigma_only) wants the
// 93-float embedding of every point in HBM and walks all 151 stages; here a point's coordinates are all that is read (the grid reads three
// axis entries), the xyz embedding is built in registers as the renderers build it (posenc_regs16), every tile walks the trunk only
// (WeightPipe16T<true>, passes0 = passes = 1: 124 of the 151 stages, the prefetcher turns to the stream's base behind xyz_encoding_8) and one
// float per point leaves.  No direction embedding, no feature accumulator.
// The arithmetic is the stand-alone route's: posenc_regs16 is the routine pack.hip's posenc uses below |v| = 64, and mlp_tile16's trunk walk is
// the full walk's code up to the sigma head -- sigma is bit-identical to crnerf_posenc_f32 + crnerf_mlp_forward_f32(sigma_only) there
// (tests/test_gpu_geometry.py).
// Schedule levers (mlp_core16.h): both taken as the inference kernels ship them (CRNERF_CORE16_LAG, CRNERF_CORE16_PRIO).
#include <hip/hip_runtime.h>
#include "kernels.h"
#include "launch.h"
#include "mlp_core16.h"

namespace crnerf {

// Point sources: coordinates of flat point i < n (n <= 2^31 - 1, so i and everything derived from it fit 32 bits; the row offset is formed in 64)
struct PointList16 {
  const float* xyz;
  __device__ __forceinline__ void get(uint32_t i, float& x, float& y, float& z) const {
    const float* row = xyz + (size_t)i * 3;
    x = row[0]; y = row[1]; z = row[2];
  }
};
struct GridAxes16 {   // i = ix + nx * (iy + ny * iz): x fastest
  const float* xs; const float* ys; const float* zs;
  uint32_t nx, ny;
  __device__ __forceinline__ void get(uint32_t i, float& x, float& y, float& z) const {
    const uint32_t t = i / nx, ix = i - t * nx;
    const uint32_t iz = t / ny, iy = t - iz * ny;
    x = xs[ix]; y = ys[iy]; z = zs[iz];
  }
};

template <class SRC>
__device__ __forceinline__ void sigma_query16_body(const char* __restrict__ packed, const SRC& src, float* __restrict__ sigma_out, uint32_t n, int iters) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  lds_char* lds = (lds_char*)smem;
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int p = lane & 15, g = lane >> 4;

  load_consts(lds, packed, packed);
  WeightPipe16T<true, CRNERF_CORE16_LAG, CRNERF_CORE16_PRIO != 0> pipe;
  pipe.start(lds, packed + CONST_BYTES, packed + CONST_BYTES, 1, 1, lane, wave);   // one model, every walk a trunk walk
  f32x4 q[V16_AHEAD];
  pipe.prime(q);
  PhaseTimer tm;
  tm.start(false);
  const DirLds nodir{nullptr};   // the trunk walk leaves in front of dir_encoding: never read

#pragma unroll 1
  for (int it = 0; it < iters; ++it) {
    // < n + 128 * gridDim.x <= 2^31 + 2^15: unsigned 32-bit holds it (all eight waves walk, also when their tile is past the end)
    const uint32_t i = (((uint32_t)it * gridDim.x + blockIdx.x) * V16_WAVES + wave) * 16u + p;
    const bool valid = i < n;
    float x, y, z;
    src.get(valid ? i : 0u, x, y, z);
    f32x4 pe[6], feat[4];
    posenc_regs16<XYZ_FREQS, 6>(x, y, z, g, pe);
    float sigma;
    mlp_tile16(pipe, 0, pe, nodir, feat, sigma, g, q, tm);
    if (valid && g == 0) sigma_out[i] = sigma;
  }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
}

__global__ __launch_bounds__(512, 2) void sigma_points16_kernel(const char* __restrict__ packed, PointList16 src, float* __restrict__ sigma, uint32_t n, int iters) {
  sigma_query16_body(packed, src, sigma, n, iters);
}
__global__ __launch_bounds__(512, 2) void sigma_grid16_kernel(const char* __restrict__ packed, GridAxes16 src, float* __restrict__ sigma, uint32_t n, int iters) {
  sigma_query16_body(packed, src, sigma, n, iters);
}

// n in [1, 2^31 - 1] (abi.hip has checked)
int launch_sigma_points16(const void* packed, const float* xyz, float* sigma, long n, hipStream_t stream) {
  const GridPlan plan = plan_grid((n + 127) / 128);   // 128 points per workgroup-iteration (8 waves x 16)
  return launch_kernel(sigma_points16_kernel, "sigma_points16_kernel", plan.grid, 512, LDS_SCRATCH, stream, (const char*)packed, PointList16{xyz}, sigma,
                       (uint32_t)n, plan.iters);
}
int launch_sigma_grid16(const void* packed, const float* xs, const float* ys, const float* zs, int nx, int ny, int nz, float* sigma, hipStream_t stream) {
  const long n = (long)nx * ny * nz;
  const GridPlan plan = plan_grid((n + 127) / 128);
  return launch_kernel(sigma_grid16_kernel, "sigma_grid16_kernel", plan.grid, 512, LDS_SCRATCH, stream, (const char*)packed,
                       GridAxes16{xs, ys, zs, (uint32_t)nx, (uint32_t)ny}, sigma, (uint32_t)n, plan.iters);
}

}  // namespace crnerf

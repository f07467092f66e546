// Density query on the bf16 pair core (mlp_core_bf16p.h): sigma of NeRF_sigma at points that do not come from rays -- a point list xyz[n][3], or
// the nodes of a grid given by three axis arrays (include/crnerf_geometry.h), in the mixed-precision semantics of include/crnerf.h "bf16".  A
// point's coordinates are all that is read (the grid reads three axis entries), the xyz embedding is built in registers as the fused renderer
// builds it (posenc_b), every 32-point tile is a trunk walk (PWalk<TRUNKB_USED, PH>: layers 1..8 + static_sigma, 992 of the 1,208 fragments) and
// one float per point leaves.  No direction embedding, no feature accumulator, no embedded row in HBM.
// Ring phase (mlp_core_bf16p.h "Trunk walk"): a trunk walk is 62 stages = half a turn of the four-slot ring, so the kernel keeps the phase of the
// next tile (0 or 2) in a scalar, toggles it once per iteration and branches between the two instantiations of the tile, as the lean renderer
// does for its coarse tiles (render_fused_bf16p.hip).  All eight waves walk every iteration, also when their tile is past the end: the ring's
// barriers need identical control flow.
#include <hip/hip_runtime.h>
#include "kernels.h"
#include "launch.h"
#include "mlp_core_bf16p.h"

namespace crnerf {

// Point sources: coordinates of flat point i < n (n <= 2^31 - 1, so i and everything derived from it fit 32 bits; the row offset is formed in 64)
struct PointListP {
  const float* xyz;
  __device__ __forceinline__ void get(uint32_t i, float& x, float& y, float& z) const {
    const float* row = xyz + (size_t)i * 3;
    x = row[0]; y = row[1]; z = row[2];
  }
};
struct GridAxesP {   // i = ix + nx * (iy + ny * iz): x fastest
  const float* xs; const float* ys; const float* zs;
  uint32_t nx, ny;
  __device__ __forceinline__ void get(uint32_t i, float& x, float& y, float& z) const {
    const uint32_t t = i / nx, ix = i - t * nx;
    const uint32_t iz = t / ny, iy = t - iz * ny;
    x = xs[ix]; y = ys[iy]; z = zs[iz];
  }
};

template <class SRC>
__device__ __forceinline__ void sigma_query_bf16p_body(const char* __restrict__ packed, const SRC& src, float* __restrict__ sigma_out, uint32_t n, int iters) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  lds_char* lds = (lds_char*)smem;
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int p = lane & 31, h = lane >> 5;

  load_consts(lds, packed, packed);
  WeightPipeP pipe;
  pipe.start(lds, packed + CONST_BYTES, packed + CONST_BYTES, 0, lane, wave);
  u32x4 q[B_AHEAD];
  pipe.prime(q);
  PhaseTimer tm;
  tm.start(false);
  NoSaveP sv;
  int ring_ph = 0;   // the ring phase of the next tile (scalar; 0 or 2)

#pragma unroll 1
  for (int it = 0; it < iters; ++it) {
    // < n + 256 * gridDim.x <= 2^31 + 2^16: unsigned 32-bit holds it
    const uint32_t i = (((uint32_t)it * gridDim.x + blockIdx.x) * P_WAVES + wave) * 32u + p;
    const bool valid = i < n;
    float x, y, z;
    src.get(valid ? i : 0u, x, y, z);
    u32x4 pe[KS_XYZ];
    posenc_b<XYZ_FREQS, KS_XYZ>(x, y, z, h, pe);
    f32x16 feat[2];   // the trunk walk zeroes it; never read
    float sigma;
    // the trunk walk reads no direction embedding: `lds` stands in for the pointer
    if (ring_ph) mlp_tile_p<PWalk<TRUNKB_USED, 2>>(pipe, 0, 0, pe, lds, feat, sigma, h, q, tm, sv);
    else mlp_tile_p<PWalk<TRUNKB_USED, 0>>(pipe, 0, 0, pe, lds, feat, sigma, h, q, tm, sv);
    ring_ph ^= 2;
    if (valid && h == 0) sigma_out[i] = sigma;
  }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
}

__global__ __launch_bounds__(512, 2) void sigma_points_bf16p_kernel(const char* __restrict__ packed, PointListP src, float* __restrict__ sigma, uint32_t n, int iters) {
  sigma_query_bf16p_body(packed, src, sigma, n, iters);
}
__global__ __launch_bounds__(512, 2) void sigma_grid_bf16p_kernel(const char* __restrict__ packed, GridAxesP src, float* __restrict__ sigma, uint32_t n, int iters) {
  sigma_query_bf16p_body(packed, src, sigma, n, iters);
}

// n in [1, 2^31 - 1] (abi.hip has checked)
int launch_sigma_points_bf16p(const void* packed, const float* xyz, float* sigma, long n, hipStream_t stream) {
  const GridPlan plan = plan_grid((n + 255) / 256);   // 256 points per workgroup-iteration (eight 32-point tiles)
  return launch_kernel(sigma_points_bf16p_kernel, "sigma_points_bf16p_kernel", plan.grid, 512, LDS_SCRATCH_P, stream, (const char*)packed, PointListP{xyz}, sigma,
                       (uint32_t)n, plan.iters);
}
int launch_sigma_grid_bf16p(const void* packed, const float* xs, const float* ys, const float* zs, int nx, int ny, int nz, float* sigma, hipStream_t stream) {
  const long n = (long)nx * ny * nz;
  const GridPlan plan = plan_grid((n + 255) / 256);
  return launch_kernel(sigma_grid_bf16p_kernel, "sigma_grid_bf16p_kernel", plan.grid, 512, LDS_SCRATCH_P, stream, (const char*)packed,
                       GridAxesP{xs, ys, zs, (uint32_t)nx, (uint32_t)ny}, sigma, (uint32_t)n, plan.iters);
}

}  // namespace crnerf

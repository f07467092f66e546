// Scene bounds: one near and one far bound per image = two percentiles of the camera-space depth of every point of the
// sparse model that lies in front of that camera.
//
// Reference: PhototourismDataset.read_meta, datasets/phototourism_mask_grid_sample.py:130-137 -- per image (xyz_world_h @ w2c.T)[:, 2],
//            the rows with depth > 0, np.percentile(depths, 0.1) and np.percentile(depths, 99.9).
// Restated (include/crnerf.h carries the definition): depth = ((x r20 + y r21) + z r22) + t2 in float64, separate multiplies and adds;
// in front = the depth's 64 bits b satisfy 0 < b <= 0x7FF0000000000000 (positive, denormals and +inf included; +-0, negatives and NaN
// excluded -- decided on the bits, the unit is compiled with -fno-honor-nans); with n in front and s their sorted depths the percentile at
// fraction f = q / 100 is numpy's linear method: v = f (n - 1), lo = floor(v), g = v - lo, a = s[lo], b = s[min(lo + 1, n - 1)],
// d = b - a, a + d g when g < 0.5, else b - d (1 - g).
//
// One workgroup per image.  A positive double orders like its bit pattern, so the four order statistics an image needs (lo, lo + 1 of
// either percentile) are found by an MSB-first radix select on the 63 magnitude bits: six passes of 11/11/11/10/10/10 bits, each streaming
// the points, recomputing the depth (nothing is stored per point) and counting, per rank, the next digit of the depths that share the
// rank's bits so far -- integer LDS atomics, so the counts and with them every output bit do not depend on the order of arrival.  Ranks
// that still share their bits share one histogram.  Pass 0 (the exponent) also counts n, from which the ranks follow.
// No roofline is claimed: the point cloud (24 B per point) is re-read six times per image from the caches; the measured rate is in
// profiles/r11/scene_bounds.txt.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "kernels.h"

namespace crnerf {

constexpr int SB_THREADS = 256;
constexpr int SB_WAVES = SB_THREADS / 64;
constexpr int SB_RANKS = 4;                     // s[lo], s[lo + 1] of q_lo, then of q_hi
constexpr int SB_BINS = 2048;                   // 11 bits, the widest digit
constexpr int SB_PASSES = 6;
constexpr int SB_PER_THREAD = SB_BINS / SB_THREADS;      // bins one thread sums
constexpr int SB_PER_LANE = SB_BINS / 64;                // bins one lane of the scanning wave covers
constexpr uint64_t SB_INF_BITS = 0x7FF0000000000000ull;
constexpr uint64_t SB_NAN_BITS = 0x7FF8000000000000ull;
static_assert(SB_WAVES == SB_RANKS, "the digit search runs one wave per rank");
static_assert(3 * 11 + 3 * 10 == 63, "the passes cover the 63 magnitude bits");

__device__ __forceinline__ int sb_width(int pass) { return pass < 3 ? 11 : 10; }

__global__ __launch_bounds__(SB_THREADS) void scene_bounds_kernel(const double* __restrict__ xyz, int n_points, const double* __restrict__ rows,
                                                                  double f_lo, double f_hi, double* __restrict__ nears,
                                                                  double* __restrict__ fars, int* __restrict__ counts) {
  __shared__ uint32_t hist[SB_RANKS][SB_BINS];
  __shared__ uint32_t part[SB_RANKS][SB_THREADS];
  __shared__ uint64_t s_prefix[SB_RANKS];       // the bits of rank j's depth above the current pass
  __shared__ uint32_t s_rank[SB_RANKS];         // rank j among the depths that share s_prefix[j]
  __shared__ int s_owner[SB_RANKS];             // the first rank with the same prefix: the histogram rank j reads
  __shared__ double s_g[2];
  __shared__ uint32_t s_n;
  const int tid = threadIdx.x, img = blockIdx.x;
  const double r0 = rows[4 * (size_t)img], r1 = rows[4 * (size_t)img + 1], r2 = rows[4 * (size_t)img + 2], t2 = rows[4 * (size_t)img + 3];
  if (tid < SB_RANKS) { s_prefix[tid] = 0; s_rank[tid] = 0; s_owner[tid] = 0; }
  if (tid == 0) s_n = 0;
  int hi_shift = 63;                            // pass 0: the bit above is the sign, 0 for every depth in front
  for (int pass = 0; pass < SB_PASSES; ++pass) {
    const int width = sb_width(pass), lo_shift = hi_shift - width;
    const uint32_t mask = (1u << width) - 1u;
    for (int k = tid; k < SB_RANKS * SB_BINS; k += SB_THREADS) (&hist[0][0])[k] = 0;
    __syncthreads();
    const uint64_t p0 = s_prefix[0], p1 = s_prefix[1], p2 = s_prefix[2], p3 = s_prefix[3];
    const bool own1 = s_owner[1] == 1, own2 = s_owner[2] == 2, own3 = s_owner[3] == 3;
    uint32_t seen = 0;
    for (int i = tid; i < n_points; i += SB_THREADS) {
      const double* p = xyz + 3 * (size_t)i;
      const double z = ((p[0] * r0 + p[1] * r1) + p[2] * r2) + t2;
      const uint64_t b = (uint64_t)__double_as_longlong(z);
      if (b - 1ull < SB_INF_BITS) {             // 0 < b <= +inf
        ++seen;
        const uint64_t top = b >> hi_shift;
        const uint32_t digit = (uint32_t)(b >> lo_shift) & mask;
        if (top == p0) atomicAdd(&hist[0][digit], 1u);
        if (own1 && top == p1) atomicAdd(&hist[1][digit], 1u);
        if (own2 && top == p2) atomicAdd(&hist[2][digit], 1u);
        if (own3 && top == p3) atomicAdd(&hist[3][digit], 1u);
      }
    }
    if (pass == 0 && seen) atomicAdd(&s_n, seen);
    __syncthreads();
    if (pass == 0) {
      const uint32_t n = s_n;
      if (n == 0) {                             // the same in every thread: nothing in front of this camera
        if (tid == 0) {
          nears[img] = __longlong_as_double((long long)SB_NAN_BITS);
          fars[img] = __longlong_as_double((long long)SB_NAN_BITS);
          counts[img] = 0;
        }
        return;
      }
      if (tid < 2) {                            // numpy's virtual index of either percentile
        const double v = (tid ? f_hi : f_lo) * (double)(n - 1u);
        const double fl = floor(v);
        const uint32_t lo = min((uint32_t)fl, n - 1u);
        s_g[tid] = v - fl;
        s_rank[2 * tid] = lo;
        s_rank[2 * tid + 1] = min(lo + 1u, n - 1u);
      }
    }
    // every thread sums its bins of the four histograms, then wave j finds rank j's digit: a scan over the lanes' 32-bin sums, a walk inside
    for (int j = 0; j < SB_RANKS; ++j) {
      uint32_t c = 0;
#pragma unroll
      for (int k = 0; k < SB_PER_THREAD; ++k) c += hist[j][SB_PER_THREAD * tid + k];
      part[j][tid] = c;
    }
    __syncthreads();
    const int j = tid >> 6, lane = tid & 63;
    const int o = s_owner[j];
    const uint32_t r = s_rank[j];
    uint32_t c = 0;
#pragma unroll
    for (int k = 0; k < SB_THREADS / 64; ++k) c += part[o][(SB_THREADS / 64) * lane + k];
    uint32_t incl = c;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
      const uint32_t up = __shfl_up(incl, d, 64);
      if (lane >= d) incl += up;
    }
    const uint32_t excl = incl - c;
    const unsigned long long found = __ballot(r >= excl && r < incl);
    const int src = found ? __ffsll((long long)found) - 1 : 0;      // exactly one lane holds r: r < the count under the prefix
    uint32_t below = __shfl(excl, src, 64);
    int digit = SB_PER_LANE * src + SB_PER_LANE - 1;
    for (int k = 0; k < SB_PER_LANE; ++k) {
      const uint32_t h = hist[o][SB_PER_LANE * src + k];
      if (r < below + h) { digit = SB_PER_LANE * src + k; break; }
      below += h;
    }
    const uint64_t prefix = (s_prefix[j] << width) | (uint64_t)digit;
    __syncthreads();                            // every wave has read the owners, prefixes and ranks of this pass
    if (lane == 0) { s_prefix[j] = prefix; s_rank[j] = r - below; }
    __syncthreads();
    if (tid < SB_RANKS) {
      int first = tid;
      for (int k = tid - 1; k >= 0; --k)
        if (s_prefix[k] == s_prefix[tid]) first = k;
      s_owner[tid] = first;
    }
    hi_shift = lo_shift;
    // the zeroing loop's barrier at the top of the next pass orders s_owner
  }
  __syncthreads();
  if (tid < 2) {                                // the prefixes are the depths: numpy's _lerp, in its order
    const double a = __longlong_as_double((long long)s_prefix[2 * tid]), b = __longlong_as_double((long long)s_prefix[2 * tid + 1]);
    const double g = s_g[tid], d = b - a;
    const double res = g < 0.5 ? a + d * g : b - d * (1.0 - g);
    (tid ? fars : nears)[img] = res;
  }
  if (tid == 0) counts[img] = (int)s_n;
}

size_t scene_bounds_workspace_bytes(int n_images, int n_points) {
  (void)n_images; (void)n_points;
  return 0;                                     // the histograms live in LDS and no depth is stored
}

int launch_scene_bounds(const double* xyz, int n_points, const double* rows, int n_images, double f_lo, double f_hi, double* nears,
                        double* fars, int* counts, void* workspace, hipStream_t stream) {
  (void)workspace;
  hipLaunchKernelGGL(scene_bounds_kernel, dim3(n_images), dim3(SB_THREADS), 0, stream, xyz, n_points, rows, f_lo, f_hi, nears, fars, counts);
  return check_launch("scene_bounds");
}

}  // namespace crnerf

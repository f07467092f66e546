// What the mesh units (mesh.hip, mesh_parts.hip, mesh_simplify.hip, mesh_smooth.hip) share (DESIGN 3.6 "the mesh scan"): the two-level exclusive
// scan that turns per-entry counts into output offsets without an atomic, the merge of a wave's runs of equal ids in front of an atomic add, the
// face load that drops a face with an id outside [0, V), and the host checks and launch step of their entry points.
//
// The scan.  A list of n entries is cut into blocks of MESH_SCAN = 1,024.  A workgroup of 256 threads, MESH_PER = 4 consecutive entries each,
// scans its block (block_scan_exclusive) and leaves every entry's offset inside the block and the block's total; then ONE workgroup of 1,024
// threads (mesh_block_scan_kernel) walks the block totals in chunks of MESH_SCAN with a running 64-bit carry and leaves exclusive block bases
// in place and the grand total.  The offset of entry i is base[i >> MESH_SCAN_SHIFT] + loc[i]; no launch waits on another workgroup.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/crnerf.h"
#include "kernels.h"

namespace crnerf {

constexpr int MESH_SCAN = 1024;                 // entries per scan workgroup = per block base
constexpr int MESH_SCAN_SHIFT = 10;
constexpr int MESH_SCAN_WAVES = MESH_SCAN / 64;
constexpr int MESH_PER = 4;                     // consecutive entries per thread of a block's scan
constexpr int MESH_PER_THREADS = MESH_SCAN / MESH_PER;
constexpr int MESH_PER_WAVES = MESH_PER_THREADS / 64;
constexpr int MESH_THREADS = 256;               // the per-entry kernels
constexpr int64_t MESH_MAX = 0x7fffffffLL;
static_assert((1 << MESH_SCAN_SHIFT) == MESH_SCAN, "block of an entry = entry >> MESH_SCAN_SHIFT");
static_assert(MESH_SCAN < 65536, "an offset inside a block is kept in 16 bits");

__host__ __device__ inline uint32_t scan_blocks(uint32_t n) { return (n + MESH_SCAN - 1) >> MESH_SCAN_SHIFT; }

// ---------------------------------------------------------------------------------------------------------------- scans
// inclusive sum of x over the lanes 0 .. lane; every lane takes part
template <class T>
__device__ __forceinline__ T wave_scan_inclusive(T x, uint32_t lane) {
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const T up = __shfl_up(x, d, 64);
    if (lane >= (uint32_t)d) x += up;
  }
  return x;
}

// Exclusive sum of `own` over the threads below this one in a workgroup of WAVES waves, and the workgroup's total: wave totals through
// wave_sum[WAVES] in LDS.  Every thread takes part.  REUSED: wave_sum was read by an earlier scan of this kernel, which the leading barrier lets
// finish; a kernel's first and only scan passes false.
template <class T, int WAVES, bool REUSED>
__device__ __forceinline__ T block_scan_exclusive(T own, T* wave_sum, uint32_t lane, uint32_t wave, T& total) {
  const T incl = wave_scan_inclusive(own, lane);
  if (REUSED) __syncthreads();
  if (lane == 63) wave_sum[wave] = incl;
  __syncthreads();
  T below = 0;
  total = 0;
#pragma unroll
  for (int k = 0; k < WAVES; ++k) {
    const T s = wave_sum[k];
    if ((uint32_t)k < wave) below += s;
    total += s;
  }
  return below + incl - own;
}

// flag[j] (0 / 1) of the entries i0 .. i0 + MESH_PER - 1 of this thread, i0 = MESH_SCAN blockIdx.x + MESH_PER threadIdx.x: loc[] = their exclusive
// ranks inside the workgroup's MESH_SCAN entries (or'ed with mark where the flag is set), base[blockIdx.x] = the total
__device__ __forceinline__ void block_offsets(const uint32_t flag[MESH_PER], uint32_t i0, uint32_t n, uint16_t mark, uint16_t* __restrict__ loc,
                                              unsigned long long* __restrict__ base) {
  __shared__ uint32_t wave_sum[MESH_PER_WAVES];
  const uint32_t tid = threadIdx.x;
  uint32_t own = 0, total;
#pragma unroll
  for (int j = 0; j < MESH_PER; ++j) own += flag[j];
  uint32_t excl = block_scan_exclusive<uint32_t, MESH_PER_WAVES, false>(own, wave_sum, tid & 63, tid >> 6, total);
#pragma unroll
  for (int j = 0; j < MESH_PER; ++j) {
    if (i0 + j < n) loc[i0 + j] = (uint16_t)(excl | (flag[j] ? mark : 0));
    excl += flag[j];
  }
  if (tid == 0) base[blockIdx.x] = total;
}

// One list of block totals: a[n] becomes its exclusive scan in place, and the sum goes to sink[0 .. SINKS).  The number of sinks (0: nobody
// wants the sum, 1, or 2: counts[i] and totals[i] of mesh_simplify.hip) is part of the type, so a kernel loads and stores what it has, untested.
template <int SINKS>
struct ScanList {
  unsigned long long* a;
  uint32_t n;
  long long* sink[SINKS > 0 ? SINKS : 1];
};
template <int LISTS, int SINKS>
struct ScanLists { ScanList<SINKS> l[LISTS]; };

// ONE workgroup.  Every unit that launches this template holds its own copy; the kernel has no floating point, so the copy built under
// mesh.hip's -fhonor-nans cannot differ from the others.
template <int LISTS, int SINKS>
__global__ __launch_bounds__(MESH_SCAN) void mesh_block_scan_kernel(ScanLists<LISTS, SINKS> lists) {
  __shared__ unsigned long long wave_sum[MESH_SCAN_WAVES];
  const uint32_t tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  // every kernel argument is read here, in front of the loop: under the loop's conditions hipcc peels the first trip to hoist the loads, and
  // behind the loop thread 0 would wait for each sink pointer in turn
  unsigned long long* a[LISTS];
  long long* sink[LISTS][SINKS > 0 ? SINKS : 1];
  unsigned long long carry[LISTS];
  uint32_t n[LISTS], top = 0;
#pragma unroll
  for (int i = 0; i < LISTS; ++i) {
    a[i] = lists.l[i].a;
    n[i] = lists.l[i].n;
#pragma unroll
    for (int s = 0; s < SINKS; ++s) sink[i][s] = lists.l[i].sink[s];
    carry[i] = 0;
    top = n[i] > top ? n[i] : top;
  }
  for (uint32_t first = 0; first < top; first += MESH_SCAN) {   // (the trip count is the same in every thread: the barriers inside are uniform)
    const uint32_t j = first + tid;
    unsigned long long own[LISTS], excl[LISTS], total[LISTS];
#pragma unroll
    for (int i = 0; i < LISTS; ++i) own[i] = j < n[i] ? a[i][j] : 0ull;
#pragma unroll
    for (int i = 0; i < LISTS; ++i) excl[i] = block_scan_exclusive<unsigned long long, MESH_SCAN_WAVES, true>(own[i], wave_sum, lane, wave, total[i]);
#pragma unroll
    for (int i = 0; i < LISTS; ++i) {
      if (j < n[i]) a[i][j] = carry[i] + excl[i];
      carry[i] += total[i];
    }
  }
  if (tid == 0) {
#pragma unroll
    for (int i = 0; i < LISTS; ++i)
#pragma unroll
      for (int s = 0; s < SINKS; ++s) *sink[i][s] = (long long)carry[i];
  }
}

// ---------------------------------------------------------------------------------------------------------------- runs of equal ids in a wave
// The lanes of a wave hold consecutive entries.  The first lane of the run of equal `id`s this lane lies in, and heads: bit l is set where lane l
// starts a run.  Every lane takes part.
__device__ __forceinline__ uint32_t run_first(int32_t id, uint32_t lane, unsigned long long& heads) {
  const int32_t before = __shfl_up(id, 1, 64);
  heads = __ballot(lane == 0 || before != id);
  const unsigned long long upto = heads & (lane == 63 ? ~0ull : ((2ull << lane) - 1ull));
  return 63u - (uint32_t)__clzll((long long)upto);      // (bit 0 of heads is set: upto != 0)
}

// this lane ends its run
__device__ __forceinline__ bool run_last(unsigned long long heads, uint32_t lane) { return lane == 63 || ((heads >> (lane + 1)) & 1ull); }

// inclusive (wrapping) sum of x over the lanes first .. lane of this lane's run; every lane takes part
template <class T>
__device__ __forceinline__ T run_sum(T x, uint32_t lane, uint32_t first) {
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const T up = __shfl_up(x, d, 64);
    if (lane >= first + (uint32_t)d) x += up;
  }
  return x;
}

// ---------------------------------------------------------------------------------------------------------------- faces
// The three ids of face f and true; or -1, -1, -1 and false for a face past the end or with an id outside [0, V): nothing of such a face is used.
// The -1s are part of the contract, not a leftover: the run-merge kernels of mesh_smooth.hip go on with EVERY lane (the shuffles need them all),
// drop the bool and test id[j] >= 0 where they store, and a dropped face's -1 must end the runs of its neighbours.  f < F is tested here, so a
// caller that has tested it for a reason of its own (it writes something for a dropped face too) pays nothing for the second test.
__device__ __forceinline__ bool load_face(const int32_t* __restrict__ faces, uint32_t f, uint32_t F, uint32_t V, int32_t id[3]) {
  id[0] = id[1] = id[2] = -1;
  if (f >= F) return false;
  const int32_t a = faces[3 * (size_t)f], b = faces[3 * (size_t)f + 1], c = faces[3 * (size_t)f + 2];
  if ((uint32_t)a >= V || (uint32_t)b >= V || (uint32_t)c >= V) return false;      // (a negative id is a large unsigned one)
  id[0] = a; id[1] = b; id[2] = c;
  return true;
}

// ---------------------------------------------------------------------------------------------------------------- host
inline size_t align16(size_t v) { return (v + 15) & ~(size_t)15; }
inline uint32_t launch_blocks(uint64_t n, uint32_t per) { return (uint32_t)((n + per - 1) / per); }

inline int mesh_sizes(const char* who, int64_t V, int64_t F) {
  if (V < 0 || F < 0) return launch_fail(CRNERF_ERR_SHAPE, who, "negative size");
  if (V > MESH_MAX || F > MESH_MAX) return launch_fail(CRNERF_ERR_SHAPE, who, "more than 2^31 - 1 vertices or faces in one call");
  return 0;
}

inline int mesh_caps(const char* who, int64_t v_cap, int64_t f_cap) {
  if (v_cap < 0 || f_cap < 0) return launch_fail(CRNERF_ERR_SHAPE, who, "negative capacity");
  if (v_cap > MESH_MAX || f_cap > MESH_MAX) return launch_fail(CRNERF_ERR_SHAPE, who, "a capacity above 2^31 - 1 (faces hold int32 vertex ids)");
  return 0;
}

// No dynamic LDS, so not launch.h's launch_kernel: that one's ensure_dynamic_lds takes a mutex and asks for the device on every call.
template <class... P, class... A>
inline int mesh_launch(void (*kernel)(P...), const char* name, uint32_t grid, uint32_t block, hipStream_t stream, const A&... args) {
  hipLaunchKernelGGL(kernel, dim3(grid), dim3(block), 0, stream, args...);
  return check_launch(name);
}

// one or two lists with the same number of sinks, e.g. ScanList<1>{base, blocks, {counts}}
template <int SINKS, class... More>
inline int mesh_block_scan(hipStream_t stream, const ScanList<SINKS>& list, const More&... more) {
  constexpr int LISTS = 1 + sizeof...(More);
  return mesh_launch(mesh_block_scan_kernel<LISTS, SINKS>, "mesh_block_scan_kernel", 1, MESH_SCAN, stream, ScanLists<LISTS, SINKS>{{list, more...}});
}

}  // namespace crnerf

// for the extern "C" entries: each returns from the entry with the refusal
#define MESH_REQUIRE(p, who, name) \
  if (!(p)) return crnerf::launch_fail(CRNERF_ERR_NULL, who, name " is NULL")
#define MESH_ALIGNED(p, who) \
  if ((uintptr_t)(p) & 15u) return crnerf::launch_fail(CRNERF_ERR_CONFIG, who, "workspace must be 16-byte aligned")
#define MESH_FILL(p, byte, bytes, st, who) \
  if (hipMemsetAsync(p, byte, bytes, st) != hipSuccess) return crnerf::launch_fail(CRNERF_ERR_HIP, who, "hipMemsetAsync failed")

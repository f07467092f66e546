// Taubin smoothing and face-derived vertex normals of an indexed mesh (csrc/crnerf_mesh_smooth.h carries every rule): positions
// on a 2^30 integer lattice, neighbour sums and normal sums in 64-bit integers -- the same bytes on every run, whatever the order of the faces.
//
// Adjacency, five launches (three when F = 0) behind one fill, none of which waits on another workgroup:
//   (fill)                    deg[V] = cursor[V] = 0, h[V] = 0
//   smooth_degree_kernel      one thread per face: an invalid face is dropped before any of its ids is used; per corner deg += 2 and
//                             h += mix(next) - mix(prev), by the last lane of every run of equal ids in a wave only (the run merge of
//                             mesh_common.h: adds to one address retire one after another, about 26 ns each, profiles/r22/mesh_parts.txt, and an
//                             extracted mesh lists the fan of a vertex in neighbouring faces)
//   smooth_offsets_kernel     the block scan of mesh_common.h over deg, in 64 bits: each row's start inside its block, the block's total
//   mesh_block_scan_kernel    (mesh_common.h) the block totals: exclusive bases, no sum is kept
//   smooth_fill_kernel        one thread per face: the first lane of a run takes 2 x (run length) slots of the row with ONE add on cursor[id] and
//                             hands them out; nbr[start + slot] = next, prev.  The order inside a row follows the order the adds retire in
// Smooth: smooth_quantise_kernel (P as 16 bytes a vertex: the three lattice coordinates and, in the fourth word, the row's length -- 0 for a
// vertex that stays: a pass reads neither deg[] nor h[]); 2 x steps smooth_pass_kernel (no atomics: a thread per vertex reads its row and gathers
// P, one 16-byte load a neighbour -- what a pass pays for is cache lines looked up, a neighbour entry and a P each, not bytes --; a row longer
// than SM_LONG entries is summed by the whole wave, 64 entries a trip); smooth_output_kernel.
// Normals: (fill) nsum = 0; normals_sum_kernel, one thread per face, the run-merged 64-bit adds of above; normals_finish_kernel.
//
// Coherence.  The XCDs' L2s are not coherent for plain accesses inside one kernel (mesh_parts.hip): deg[], h[], cursor[] and nsum[] are touched
// with agent-scope atomics only inside the kernels that write them; later launches read them plainly.  nbr[] and P[] are written plainly by one
// launch and read by the next.
//
// Workspace: base[nb] (uint64) | deg[V] cursor[V] (uint32) | h[V] rowstart[V] (uint64) | P0[V] P1[V] (int32 x 4) | nsum[V][3] (int64) |
// nbr[6 F] (int32); every array on a 16-byte boundary.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include "crnerf_mesh_smooth.h"
#include "mesh_common.h"

namespace crnerf {

constexpr uint32_t SM_LONG = 64;                // entries: a longer row is summed by the wave together
constexpr int32_t SM_ONE = 1 << 30;             // the lattice: P in [0, 2^30]
constexpr int32_t SM_MAX_STEPS = 65536;

struct SmWorkspace {
  unsigned long long* base;       // [nb] block totals, then exclusive bases
  uint32_t* deg;                  // [V] entries of the row
  uint32_t* cursor;               // [V] entries filled so far
  unsigned long long* h;          // [V] sum of mix(next) - mix(prev)
  unsigned long long* rowstart;   // [V] start of the row inside its block
  int4* p0;                       // [V] x, y, z on the lattice; w: the entries of the row, 0 when the vertex stays
  int4* p1;                       // [V]
  long long* nsum;                // [V][3]
  int32_t* nbr;                   // [6 F]
};

constexpr size_t SM_WORKSPACE_PAD = 192;        // nine roundings of at most 15 bytes each, and room to spare

static SmWorkspace sm_carve(void* workspace, uint32_t V) {
  SmWorkspace w;
  char* p = (char*)workspace;
  size_t off = 0;
  w.base = (unsigned long long*)(p + off); off = align16(off + 8 * (size_t)scan_blocks(V));
  w.deg = (uint32_t*)(p + off); off = align16(off + 4 * (size_t)V);
  w.cursor = (uint32_t*)(p + off); off = align16(off + 4 * (size_t)V);
  w.h = (unsigned long long*)(p + off); off = align16(off + 8 * (size_t)V);
  w.rowstart = (unsigned long long*)(p + off); off = align16(off + 8 * (size_t)V);
  w.p0 = (int4*)(p + off); off = align16(off + 16 * (size_t)V);
  w.p1 = (int4*)(p + off); off = align16(off + 16 * (size_t)V);
  w.nsum = (long long*)(p + off); off = align16(off + 24 * (size_t)V);
  w.nbr = (int32_t*)(p + off);
  return w;
}

__device__ __forceinline__ unsigned long long sm_mix(int32_t id) {
  unsigned long long z = (unsigned long long)(uint32_t)id + 0x9E3779B97F4A7C15ull;
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}

// ---------------------------------------------------------------------------------------------------------------- adjacency
__global__ __launch_bounds__(MESH_THREADS) void smooth_degree_kernel(const int32_t* __restrict__ faces, uint32_t V, uint32_t F, uint32_t* deg,
                                                                   unsigned long long* h) {
  const uint32_t f = blockIdx.x * (uint32_t)MESH_THREADS + threadIdx.x, lane = threadIdx.x & 63;
  int32_t id[3];
  load_face(faces, f, F, V, id);
  unsigned long long m[3] = {0, 0, 0};
  if (id[0] >= 0) {
#pragma unroll
    for (int j = 0; j < 3; ++j) m[j] = sm_mix(id[j]);
  }
#pragma unroll
  for (int j = 0; j < 3; ++j) {                              // corner j: next = j + 1, prev = j + 2 (every lane runs the shuffles)
    unsigned long long heads;
    const uint32_t first = run_first(id[j], lane, heads);
    const unsigned long long sum = run_sum(m[(j + 1) % 3] - m[(j + 2) % 3], lane, first);
    if (id[j] >= 0 && run_last(heads, lane)) {               // id[j] < V
      atomicAdd(deg + id[j], 2u * (lane - first + 1u));
      atomicAdd(h + id[j], sum);
    }
  }
}

__global__ __launch_bounds__(MESH_PER_THREADS) void smooth_offsets_kernel(const uint32_t* __restrict__ deg, uint32_t V,
                                                                        unsigned long long* __restrict__ rowstart,
                                                                        unsigned long long* __restrict__ base) {
  __shared__ unsigned long long wave_sum[MESH_PER_WAVES];
  const uint32_t tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const uint32_t i0 = blockIdx.x * (uint32_t)MESH_SCAN + MESH_PER * tid;
  uint32_t d[MESH_PER];
  unsigned long long own = 0;
#pragma unroll
  for (int j = 0; j < MESH_PER; ++j) {
    d[j] = i0 + j < V ? deg[i0 + j] : 0u;
    own += d[j];
  }
  unsigned long long total;
  unsigned long long excl = block_scan_exclusive<unsigned long long, MESH_PER_WAVES, false>(own, wave_sum, lane, wave, total);
#pragma unroll
  for (int j = 0; j < MESH_PER; ++j) {
    if (i0 + j < V) rowstart[i0 + j] = excl;
    excl += d[j];
  }
  if (tid == 0) base[blockIdx.x] = total;
}

__global__ __launch_bounds__(MESH_THREADS) void smooth_fill_kernel(const int32_t* __restrict__ faces, uint32_t V, uint32_t F,
                                                                 const unsigned long long* __restrict__ base,
                                                                 const unsigned long long* __restrict__ rowstart, uint32_t* cursor,
                                                                 unsigned long long entries, int32_t* __restrict__ nbr) {
  const uint32_t f = blockIdx.x * (uint32_t)MESH_THREADS + threadIdx.x, lane = threadIdx.x & 63;
  int32_t id[3];
  load_face(faces, f, F, V, id);
#pragma unroll
  for (int j = 0; j < 3; ++j) {
    unsigned long long heads;
    const uint32_t first = run_first(id[j], lane, heads);
    const unsigned long long run = __ballot(run_last(heads, lane));      // the last lane of this lane's run: the lowest set bit at or above this lane
    const uint32_t end = (uint32_t)__ffsll((long long)(run >> lane)) - 1u + lane;
    uint32_t slot = 0;
    if (id[j] >= 0 && lane == first) slot = atomicAdd(cursor + id[j], 2u * (end - first + 1u));
    slot = __shfl(slot, (int)first, 64) + 2u * (lane - first);
    if (id[j] >= 0) {
      const unsigned long long at = base[(uint32_t)id[j] >> MESH_SCAN_SHIFT] + rowstart[id[j]] + slot;
      if (at + 1 < entries) {                                // entries = 6 F, the room nbr has; slot + 1 < deg[id] when the faces are those degree saw
        nbr[at] = id[(j + 1) % 3];
        nbr[at + 1] = id[(j + 2) % 3];
      }
    }
  }
}

// ---------------------------------------------------------------------------------------------------------------- smooth
__global__ __launch_bounds__(MESH_THREADS) void smooth_quantise_kernel(const float* __restrict__ vertices, uint32_t V, double lo0, double lo1, double lo2,
                                                                     double scale, const uint32_t* __restrict__ deg,
                                                                     const unsigned long long* __restrict__ h, int pin_border, int4* __restrict__ p) {
  const uint32_t v = blockIdx.x * (uint32_t)MESH_THREADS + threadIdx.x;
  if (v >= V) return;
  const double lo[3] = {lo0, lo1, lo2};
  int32_t q[3];
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    const float x = vertices[3 * (size_t)v + a];
    double t = ((double)x - lo[a]) * scale;
    if ((__float_as_uint(x) & 0x7fffffffu) > 0x7f800000u) t = 0.0;      // a NaN is found in the bits (the unit is built with -fno-honor-nans)
    t = fmin(fmax(t, 0.0), (double)SM_ONE);                             // the bounds are integers: clamping before rint is clamping after it
    q[a] = (int32_t)rint(t);
  }
  const uint32_t d = deg[v];
  const bool moves = d != 0 && !(pin_border && h[v] != 0ull);
  p[v] = make_int4(q[0], q[1], q[2], moves ? (int32_t)d : 0);
}

__device__ __forceinline__ int32_t sm_relax(int32_t p, long long s, uint32_t d, double w) {
  const double pf = (double)p;
  const double mean = (double)s / (double)d;
  const double diff = mean - pf;
  const double moved = pf + w * diff;
  const double r = fmin(fmax(rint(moved), 0.0), (double)SM_ONE);
  return (int32_t)r;
}

__global__ __launch_bounds__(MESH_THREADS) void smooth_pass_kernel(const int4* __restrict__ p, uint32_t V, const unsigned long long* __restrict__ base,
                                                                 const unsigned long long* __restrict__ rowstart, const int32_t* __restrict__ nbr,
                                                                 unsigned long long entries, double w, int4* __restrict__ out) {
  const uint32_t v = blockIdx.x * (uint32_t)MESH_THREADS + threadIdx.x, lane = threadIdx.x & 63;
  uint32_t d = 0;
  unsigned long long start = 0;
  int4 own = make_int4(0, 0, 0, 0);
  if (v < V) {
    own = p[v];
    d = (uint32_t)own.w;                                       // 0: the vertex stays
    start = base[v >> MESH_SCAN_SHIFT] + rowstart[v];
    if (start + d > entries) d = 0;                            // (never, for the workspace adjacency left: a row read stays inside nbr)
  }
  long long s[3] = {0, 0, 0};
  if (d <= SM_LONG) {
    for (uint32_t e = 0; e < d; e += 4) {                      // four entries, then their four gathers: the loads of a trip are in flight together
      uint32_t j[4];
#pragma unroll
      for (int i = 0; i < 4; ++i) j[i] = e + i < d ? (uint32_t)nbr[start + e + i] : 0xffffffffu;
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        if (j[i] < V) {                                        // (what fill wrote is a vertex id; a row it did not finish is not followed out of P)
          const int4 q = p[j[i]];
          s[0] += q.x; s[1] += q.y; s[2] += q.z;
        }
      }
    }
  }
  // the long rows of this wave, one after another, 64 entries a trip; every lane takes part
  unsigned long long todo = __ballot(d > SM_LONG);
  while (todo) {
    const int owner = __ffsll((long long)todo) - 1;
    todo &= todo - 1;
    const uint32_t od = __shfl(d, owner, 64);
    const unsigned long long ostart = __shfl(start, owner, 64);
    long long t[3] = {0, 0, 0};
    for (uint32_t e = lane; e < od; e += 64) {
      const uint32_t j = (uint32_t)nbr[ostart + e];
      if (j < V) {
        const int4 q = p[j];
        t[0] += q.x; t[1] += q.y; t[2] += q.z;
      }
    }
#pragma unroll
    for (int a = 0; a < 3; ++a) {
#pragma unroll
      for (int sh = 32; sh > 0; sh >>= 1) t[a] += __shfl_xor(t[a], sh, 64);
      if ((int)lane == owner) s[a] = t[a];
    }
  }
  if (v >= V) return;
  if (d != 0) {
    own.x = sm_relax(own.x, s[0], d, w);
    own.y = sm_relax(own.y, s[1], d, w);
    own.z = sm_relax(own.z, s[2], d, w);
  }
  out[v] = own;
}

__global__ __launch_bounds__(MESH_THREADS) void smooth_output_kernel(const int4* __restrict__ p, uint32_t V, double lo0, double lo1, double lo2,
                                                                   double inv_scale, float* __restrict__ out) {
  const uint32_t v = blockIdx.x * (uint32_t)MESH_THREADS + threadIdx.x;
  if (v >= V) return;
  const int4 q = p[v];
  out[3 * (size_t)v] = (float)(lo0 + (double)q.x * inv_scale);      // (2^-k: the product is ldexp's)
  out[3 * (size_t)v + 1] = (float)(lo1 + (double)q.y * inv_scale);
  out[3 * (size_t)v + 2] = (float)(lo2 + (double)q.z * inv_scale);
}

// ---------------------------------------------------------------------------------------------------------------- normals
__device__ __forceinline__ long long sm_fixed64(double c, double scale) {
  const double t = c * scale;
  const double lim = 4611686018427387904.0;                    // 2^62
  return (long long)rint(fmin(fmax(t, -lim), lim));
}

__global__ __launch_bounds__(MESH_THREADS) void normals_sum_kernel(const float* __restrict__ vertices, const int32_t* __restrict__ faces, uint32_t V,
                                                                 uint32_t F, double scale, long long* nsum) {
  const uint32_t f = blockIdx.x * (uint32_t)MESH_THREADS + threadIdx.x, lane = threadIdx.x & 63;
  int32_t id[3];
  load_face(faces, f, F, V, id);
  unsigned long long q[3] = {0, 0, 0};
  if (id[0] >= 0) {
    double a[3], e1[3], e2[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      a[k] = (double)vertices[3 * (size_t)id[0] + k];
      e1[k] = (double)vertices[3 * (size_t)id[1] + k] - a[k];
      e2[k] = (double)vertices[3 * (size_t)id[2] + k] - a[k];
    }
    q[0] = (unsigned long long)sm_fixed64(e1[1] * e2[2] - e1[2] * e2[1], scale);
    q[1] = (unsigned long long)sm_fixed64(e1[2] * e2[0] - e1[0] * e2[2], scale);
    q[2] = (unsigned long long)sm_fixed64(e1[0] * e2[1] - e1[1] * e2[0], scale);
  }
#pragma unroll
  for (int j = 0; j < 3; ++j) {
    unsigned long long heads, sum[3];
    const uint32_t first = run_first(id[j], lane, heads);
#pragma unroll
    for (int k = 0; k < 3; ++k) sum[k] = run_sum(q[k], lane, first);
    if (id[j] >= 0 && run_last(heads, lane)) {
#pragma unroll
      for (int k = 0; k < 3; ++k) atomicAdd((unsigned long long*)nsum + 3 * (size_t)id[j] + k, sum[k]);
    }
  }
}

__global__ __launch_bounds__(MESH_THREADS) void normals_finish_kernel(const long long* __restrict__ nsum, uint32_t V, float* __restrict__ out) {
  const uint32_t v = blockIdx.x * (uint32_t)MESH_THREADS + threadIdx.x;
  if (v >= V) return;
  const long long* n = nsum + 3 * (size_t)v;
  const double x = (double)n[0], y = (double)n[1], z = (double)n[2];
  const bool zero = n[0] == 0 && n[1] == 0 && n[2] == 0;
  const double len = sqrt((x * x + y * y) + z * z);
  out[3 * (size_t)v] = zero ? 0.0f : (float)(x / len);
  out[3 * (size_t)v + 1] = zero ? 0.0f : (float)(y / len);
  out[3 * (size_t)v + 2] = zero ? 0.0f : (float)(z / len);
}

}  // namespace crnerf

// ---------------------------------------------------------------------------------------------------------------- host
using namespace crnerf;

extern "C" size_t crnerf_mesh_smooth_workspace_bytes(int64_t V, int64_t F) {
  if (V <= 0 || F < 0 || V > MESH_MAX || F > MESH_MAX) return 0;
  return (size_t)8 * scan_blocks((uint32_t)V) + (size_t)80 * (size_t)V + (size_t)24 * (size_t)F + SM_WORKSPACE_PAD;
}

extern "C" int crnerf_mesh_adjacency_i32(const int32_t* faces, int64_t V, int64_t F, void* workspace, void* stream) {
  static const char* who = "mesh_adjacency";
  if (int rc = mesh_sizes(who, V, F)) return rc;
  if (V == 0) return 0;
  MESH_REQUIRE(workspace, who, "workspace");
  if (F > 0) MESH_REQUIRE(faces, who, "faces");
  MESH_ALIGNED(workspace, who);
  hipStream_t st = (hipStream_t)stream;
  const uint32_t v = (uint32_t)V, f = (uint32_t)F;
  const SmWorkspace w = sm_carve(workspace, v);
  // deg, cursor and h lie one behind the other; the roundings between them are zeroed with them
  MESH_FILL(w.deg, 0, (size_t)((char*)w.rowstart - (char*)w.deg), st, who);
  const uint32_t fblocks = launch_blocks(f, MESH_THREADS);
  if (f > 0) {
    if (int rc = mesh_launch(smooth_degree_kernel, "smooth_degree_kernel", fblocks, MESH_THREADS, st, faces, v, f, w.deg, w.h)) return rc;
  }
  if (int rc = mesh_launch(smooth_offsets_kernel, "smooth_offsets_kernel", scan_blocks(v), MESH_PER_THREADS, st, w.deg, v, w.rowstart, w.base)) return rc;
  if (int rc = mesh_block_scan(st, ScanList<0>{w.base, scan_blocks(v), {}})) return rc;
  if (f > 0)
    return mesh_launch(smooth_fill_kernel, "smooth_fill_kernel", fblocks, MESH_THREADS, st, faces, v, f, w.base, w.rowstart, w.cursor, 6ull * f, w.nbr);
  return 0;
}

extern "C" int crnerf_mesh_smooth_f32(const float* vertices, int64_t V, int64_t F, float lo0, float lo1, float lo2, int32_t k, int32_t steps,
                                      double lambda, double mu, int32_t pin_border, void* workspace, float* out_vertices, void* stream) {
  static const char* who = "mesh_smooth";
  if (int rc = mesh_sizes(who, V, F)) return rc;
  if (steps < 0) return launch_fail(CRNERF_ERR_SHAPE, who, "negative steps");
  if (steps > SM_MAX_STEPS) return launch_fail(CRNERF_ERR_SHAPE, who, "more than 65,536 steps");
  if (!std::isfinite(lambda) || fabs(lambda) > 2.0) return launch_fail(CRNERF_ERR_SHAPE, who, "a lambda that is not finite or has |lambda| > 2");
  if (!std::isfinite(mu) || fabs(mu) > 2.0) return launch_fail(CRNERF_ERR_SHAPE, who, "a mu that is not finite or has |mu| > 2");
  if (k < -100 || k > 100) return launch_fail(CRNERF_ERR_SHAPE, who, "k outside [-100, 100]");
  if (!std::isfinite(lo0) || !std::isfinite(lo1) || !std::isfinite(lo2)) return launch_fail(CRNERF_ERR_SHAPE, who, "a box origin that is not finite");
  if (V == 0) return 0;
  MESH_REQUIRE(vertices, who, "vertices"); MESH_REQUIRE(workspace, who, "workspace"); MESH_REQUIRE(out_vertices, who, "out_vertices");
  MESH_ALIGNED(workspace, who);
  hipStream_t st = (hipStream_t)stream;
  const uint32_t v = (uint32_t)V, f = (uint32_t)F;
  const SmWorkspace w = sm_carve(workspace, v);
  const uint32_t blocks = launch_blocks(v, MESH_THREADS);
  if (int rc = mesh_launch(smooth_quantise_kernel, "smooth_quantise_kernel", blocks, MESH_THREADS, st, vertices, v, (double)lo0, (double)lo1, (double)lo2,
                           ldexp(1.0, k), w.deg, w.h, pin_border ? 1 : 0, w.p0))
    return rc;
  int4* from = w.p0;
  int4* to = w.p1;
  for (int32_t pass = 0; pass < 2 * steps; ++pass) {
    if (int rc = mesh_launch(smooth_pass_kernel, "smooth_pass_kernel", blocks, MESH_THREADS, st, from, v, w.base, w.rowstart, w.nbr, 6ull * f,
                             (pass & 1) ? mu : lambda, to))
      return rc;
    int4* t = from; from = to; to = t;
  }
  return mesh_launch(smooth_output_kernel, "smooth_output_kernel", blocks, MESH_THREADS, st, from, v, (double)lo0, (double)lo1, (double)lo2, ldexp(1.0, -k),
                     out_vertices);
}

extern "C" int crnerf_mesh_vertex_normals_f32(const float* vertices, const int32_t* faces, int64_t V, int64_t F, int32_t k2, void* workspace,
                                              float* out_normals, void* stream) {
  static const char* who = "mesh_vertex_normals";
  if (int rc = mesh_sizes(who, V, F)) return rc;
  if (k2 < -300 || k2 > 300) return launch_fail(CRNERF_ERR_SHAPE, who, "k2 outside [-300, 300]");
  if (V == 0) return 0;
  MESH_REQUIRE(workspace, who, "workspace"); MESH_REQUIRE(out_normals, who, "out_normals");
  if (F > 0) { MESH_REQUIRE(vertices, who, "vertices"); MESH_REQUIRE(faces, who, "faces"); }
  MESH_ALIGNED(workspace, who);
  hipStream_t st = (hipStream_t)stream;
  const uint32_t v = (uint32_t)V, f = (uint32_t)F;
  const SmWorkspace w = sm_carve(workspace, v);
  MESH_FILL(w.nsum, 0, 24 * (size_t)V, st, who);
  if (f > 0) {
    if (int rc = mesh_launch(normals_sum_kernel, "normals_sum_kernel", launch_blocks(f, MESH_THREADS), MESH_THREADS, st, vertices, faces, v, f, ldexp(1.0, k2),
                             w.nsum))
      return rc;
  }
  return mesh_launch(normals_finish_kernel, "normals_finish_kernel", launch_blocks(v, MESH_THREADS), MESH_THREADS, st, w.nsum, v, out_normals);
}

// Connected parts of an indexed triangle mesh (include/crnerf_mesh_parts.h carries every rule): labels, sizes and a filtered copy,
// the same bytes on every run.
//
// Labelling, five launches, none of which waits on another workgroup:
//   parts_init_kernel     parent[v] = v
//   parts_union_kernel    one thread per face: an invalid face is dropped before any of its ids is used; union(a, b), union(a, c).  A union walks
//                         the two chains together (agent-scope loads), the larger end first, until they meet; a larger end that is a ROOT is
//                         hooked under the smaller end with one atomicCAS(parent[larger], larger, smaller), and the walk goes on only when that
//                         CAS lost to another thread's update.  parent[v] <= v throughout, so every chain falls and ends, and the root of a
//                         finished tree is its smallest id: the labels do not depend on the order the unions ran in.
//   parts_roots_kernel    flatten (parent[v] = root) and the block scan of mesh_common.h over the root flags
//   mesh_block_scan_kernel  (mesh_common.h) the one list of block totals: counts[0] = K
//   parts_apply_kernel    vertex_part[v] = base[block(root)] + rank[root]; face_part[f] likewise through the face's first id, -1 when invalid
// Roots are ranked in id order and a root is its part's smallest id: part ids ascend in the smallest vertex id.
//
// Coherence.  The XCDs' L2s are not coherent for plain accesses inside one kernel, so the union kernel touches parent[] with agent-scope atomics
// only (loads, the CAS, the atomicMin).  A stale value would still be harmless: parent[x] only ever moves to an ancestor of x, or -- for a root
// -- from x to something smaller, which the CAS then reports.  The other kernels use plain accesses: what they read was written by an earlier
// launch, and the flatten's own in-place writes are again ancestors.
//
// Sizes: integer atomicAdd only (exact: deterministic).  A wave takes 1,024 consecutive labels at a time, in 16 steps; at every step the lanes
// that hold the label the wave is summing are counted by a ballot into a wave-uniform register, the other labels of the step go out one add per
// distinct label, and a label that outnumbers the summed one in a step takes its place.  At most 512 workgroups walk a list and the four waves of
// a workgroup merge their sums through LDS: a mesh that is mostly one part makes at most 512 adds to that part's counter, not one per wave --
// adds to one address retire one after another, about 26 ns each (profiles/r22/mesh_parts.txt).
//
// Selection: parts_keep_kernel (block scan of the keep flags, vertices and faces in a launch each), mesh_block_scan_kernel over both lists of
// block totals, parts_emit_kernel (rows copied as 32-bit words, ids remapped through the vertex offsets).
//
// Workspace: vbase[nbV] fbase[nbF] (uint64) | parent[V] (int32) | vloc[V] | floc[F] (uint16), every array on a 16-byte boundary.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/crnerf_mesh_parts.h"
#include "mesh_common.h"

namespace crnerf {

constexpr int MP_SIZE_STEPS = 16;               // a wave of the size pass takes 64 * 16 labels at a time
constexpr int MP_SIZE_BLOCKS = 512;             // and at most this many workgroups share a list: adds to ONE address cost ~26 ns each, one after another

struct MpWorkspace {
  unsigned long long* vbase;      // [nbV] block totals, then exclusive bases
  unsigned long long* fbase;      // [nbF]
  int32_t* parent;                // [V]
  uint16_t* vloc;                 // [V] flagged entries of the block below this one
  uint16_t* floc;                 // [F]
};

constexpr size_t MP_WORKSPACE_PAD = 64;         // four roundings, at most 15 bytes each

static MpWorkspace mp_carve(void* workspace, uint32_t V, uint32_t F) {
  MpWorkspace w;
  char* p = (char*)workspace;
  size_t off = 0;
  w.vbase = (unsigned long long*)(p + off); off += 8 * (size_t)scan_blocks(V);
  w.fbase = (unsigned long long*)(p + off); off = align16(off + 8 * (size_t)scan_blocks(F));
  w.parent = (int32_t*)(p + off); off = align16(off + 4 * (size_t)V);
  w.vloc = (uint16_t*)(p + off); off = align16(off + 2 * (size_t)V);
  w.floc = (uint16_t*)(p + off);
  return w;
}

// ---------------------------------------------------------------------------------------------------------------- union-find
__global__ __launch_bounds__(MESH_THREADS) void parts_init_kernel(int32_t* __restrict__ parent, uint32_t V) {
  const uint32_t i = blockIdx.x * (uint32_t)MESH_THREADS + threadIdx.x;
  if (i < V) parent[i] = (int32_t)i;
}

__device__ __forceinline__ int32_t mp_load(int32_t* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// The two chains are walked together, always the LARGER end one link up, until they meet -- at a common ancestor, usually far below the root: the
// ids of a face are neighbours, and so are their chains.  A finished part's root is then read by nobody (every find ending on parent[root] made
// that one line the whole kernel's bottleneck: profiles/r22/mesh_parts.txt).  A larger end that is a root is hooked under the smaller end --
// which, being smaller, is not in its tree --; a CAS that loses returns the link another thread wrote, and the walk goes on from there.
// Afterwards both starting points are moved to the meeting point with atomicMin: an ancestor of both, and a link only ever falls.
__device__ __forceinline__ void mp_union(int32_t* parent, const int32_t a0, const int32_t b0) {
  int32_t a = a0, b = b0;
  while (a != b) {
    if (a < b) { const int32_t t = a; a = b; b = t; }      // a: the larger end
    int32_t p = mp_load(parent + a);
    if (p == a) {
      const int32_t old = atomicCAS(parent + a, a, b);
      if (old == a) { a = b; break; }                       // hooked: the chains now meet at b
      p = old;                                              // another thread hooked a first
    }
    a = p;                                                  // p < a: the walk falls, so it ends
  }
  if (a < a0) atomicMin(parent + a0, a);                    // (a proper ancestor: a0 is no root, no CAS targets it)
  if (a < b0) atomicMin(parent + b0, a);
}

__global__ __launch_bounds__(MESH_THREADS) void parts_union_kernel(const int32_t* __restrict__ faces, uint32_t V, uint32_t F, int32_t* parent) {
  const uint32_t f = blockIdx.x * (uint32_t)MESH_THREADS + threadIdx.x;
  int32_t id[3];
  if (!load_face(faces, f, F, V, id)) return;
  const int32_t a = id[0], b = id[1], c = id[2];
  if (a != b) mp_union(parent, a, b);
  if (a != c && b != c) mp_union(parent, a, c);
}

// ---------------------------------------------------------------------------------------------------------------- flags -> offsets inside a block
__global__ __launch_bounds__(MESH_PER_THREADS) void parts_roots_kernel(int32_t* parent, uint32_t V, uint16_t* __restrict__ loc,
                                                                      unsigned long long* __restrict__ base) {
  const uint32_t i0 = blockIdx.x * (uint32_t)MESH_SCAN + MESH_PER * threadIdx.x;
  uint32_t flag[MESH_PER];
#pragma unroll
  for (int j = 0; j < MESH_PER; ++j) {
    flag[j] = 0;
    const uint32_t i = i0 + j;
    if (i < V) {
      int32_t r = (int32_t)i, p = parent[i];
      while (p != r) { r = p; p = parent[r]; }      // strictly falling: it ends
      parent[i] = r;
      flag[j] = (uint32_t)r == i;
    }
  }
  block_offsets(flag, i0, V, 0, loc, base);
}

__device__ __forceinline__ bool mp_kept(int32_t label, uint32_t K, const uint8_t* __restrict__ keep) {
  return (uint32_t)label < K && keep[label] != 0;   // (a negative label is a large unsigned one: keep[] is read inside [0, K) only)
}

__global__ __launch_bounds__(MESH_PER_THREADS) void parts_keep_kernel(const int32_t* __restrict__ labels, uint32_t n, uint32_t K,
                                                                     const uint8_t* __restrict__ keep, uint16_t* __restrict__ loc,
                                                                     unsigned long long* __restrict__ base) {
  const uint32_t i0 = blockIdx.x * (uint32_t)MESH_SCAN + MESH_PER * threadIdx.x;
  uint32_t flag[MESH_PER];
#pragma unroll
  for (int j = 0; j < MESH_PER; ++j) flag[j] = (i0 + j < n && mp_kept(labels[i0 + j], K, keep)) ? 1u : 0u;
  block_offsets(flag, i0, n, 0, loc, base);
}

// ---------------------------------------------------------------------------------------------------------------- labels
__global__ __launch_bounds__(MESH_THREADS) void parts_apply_kernel(const int32_t* __restrict__ faces, uint32_t V, uint32_t F, MpWorkspace w,
                                                                 int32_t* __restrict__ vertex_part, int32_t* __restrict__ face_part) {
  const uint32_t i = blockIdx.x * (uint32_t)MESH_THREADS + threadIdx.x;
  if (i < V) {
    const uint32_t r = (uint32_t)w.parent[i];
    vertex_part[i] = (int32_t)(w.vbase[r >> MESH_SCAN_SHIFT] + w.vloc[r]);
  }
  if (i < F && face_part) {                     // (i < F here as well: a dropped face below F still gets its -1)
    int32_t id[3], part = -1;
    if (load_face(faces, i, F, V, id)) {
      const uint32_t r = (uint32_t)w.parent[id[0]];
      part = (int32_t)(w.vbase[r >> MESH_SCAN_SHIFT] + w.vloc[r]);
    }
    face_part[i] = part;
  }
}

// ---------------------------------------------------------------------------------------------------------------- sizes
__global__ __launch_bounds__(MESH_THREADS) void parts_sizes_kernel(const int32_t* __restrict__ labels, uint32_t n, uint32_t K, int32_t* out) {
  __shared__ int32_t wave_label[MESH_THREADS / 64];
  __shared__ uint32_t wave_acc[MESH_THREADS / 64];
  const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const uint64_t waves = (uint64_t)gridDim.x * (MESH_THREADS / 64);
  int32_t acc_label = -1;         // wave-uniform: the label this wave sums in a register, and its sum
  uint32_t acc = 0;
  for (uint64_t chunk = (uint64_t)blockIdx.x * (MESH_THREADS / 64) + wave; chunk * (64 * MP_SIZE_STEPS) < n; chunk += waves) {
    const uint64_t wave_first = chunk * (64 * MP_SIZE_STEPS);
    int32_t mine[MP_SIZE_STEPS];  // every load first: one memory latency a chunk, not sixteen
#pragma unroll
    for (int j = 0; j < MP_SIZE_STEPS; ++j) {
      const uint64_t i = wave_first + 64 * j + lane;
      mine[j] = i < n ? labels[i] : -1;
    }
#pragma unroll
    for (int j = 0; j < MP_SIZE_STEPS; ++j) {
      const int32_t label = mine[j];
      const bool ok = (uint32_t)label < K;
      uint32_t c0 = (uint32_t)__popcll(__ballot(ok && label == acc_label));      // (acc_label = -1: no lane, -1 is not ok)
      acc += c0;
      unsigned long long todo = __ballot(ok && label != acc_label);
      while (todo) {              // one round per further label of the step; todo is the same in every lane
        const int leader = __ffsll((long long)todo) - 1;
        const int32_t ll = __shfl(label, leader, 64);
        const unsigned long long same = __ballot(ok && label == ll) & todo;
        const uint32_t c = (uint32_t)__popcll(same);
        if (c > c0) {             // more of these than of the summed label in this step: sum this one from here on
          if (acc && lane == 0) atomicAdd(out + acc_label, (int32_t)acc);
          acc_label = ll;
          acc = c0 = c;
        } else if (lane == (uint32_t)leader) {
          atomicAdd(out + ll, (int32_t)c);      // ll < K: the label passed `ok`
        }
        todo &= ~same;
      }
    }
  }
  if (lane == 0) { wave_label[wave] = acc_label; wave_acc[wave] = acc; }
  __syncthreads();
  if (threadIdx.x == 0) {         // the waves of a workgroup mostly sum the same label: one add for all of them
    for (int a = 0; a < MESH_THREADS / 64; ++a) {
      uint32_t total = wave_acc[a];
      if (!total) continue;
      for (int b = a + 1; b < MESH_THREADS / 64; ++b)
        if (wave_label[b] == wave_label[a]) { total += wave_acc[b]; wave_acc[b] = 0; }
      atomicAdd(out + wave_label[a], (int32_t)total);
    }
  }
}

// ---------------------------------------------------------------------------------------------------------------- emit
__global__ __launch_bounds__(MESH_THREADS) void parts_emit_kernel(const uint32_t* __restrict__ vertices, const uint32_t* __restrict__ normals,
                                                                const int32_t* __restrict__ faces, const int32_t* __restrict__ vertex_part,
                                                                const int32_t* __restrict__ face_part, uint32_t V, uint32_t F, uint32_t K,
                                                                const uint8_t* __restrict__ keep, MpWorkspace w, long long v_cap, long long f_cap,
                                                                uint32_t* __restrict__ out_vertices, uint32_t* __restrict__ out_normals,
                                                                int32_t* __restrict__ out_faces) {
  const uint32_t i = blockIdx.x * (uint32_t)MESH_THREADS + threadIdx.x;
  if (i < V && v_cap > 0 && mp_kept(vertex_part[i], K, keep)) {
    const long long id = (long long)(w.vbase[i >> MESH_SCAN_SHIFT] + w.vloc[i]);
    if (id < v_cap) {
#pragma unroll
      for (int k = 0; k < 3; ++k) out_vertices[3 * id + k] = vertices[3 * (size_t)i + k];
      if (normals) {
#pragma unroll
        for (int k = 0; k < 3; ++k) out_normals[3 * id + k] = normals[3 * (size_t)i + k];
      }
    }
  }
  if (i < F && f_cap > 0 && mp_kept(face_part[i], K, keep)) {
    const long long id = (long long)(w.fbase[i >> MESH_SCAN_SHIFT] + w.floc[i]);
    if (id < f_cap) {
#pragma unroll
      for (int k = 0; k < 3; ++k) {
        const uint32_t q = (uint32_t)faces[3 * (size_t)i + k];
        out_faces[3 * id + k] = q < V ? (int32_t)(w.vbase[q >> MESH_SCAN_SHIFT] + w.vloc[q]) : -1;
      }
    }
  }
}

// ---------------------------------------------------------------------------------------------------------------- host
static int mp_parts(const char* who, int64_t V, int64_t K) {
  if (K < 0) return launch_fail(CRNERF_ERR_SHAPE, who, "negative size");
  if (K > V) return launch_fail(CRNERF_ERR_SHAPE, who, "more parts than vertices (K > V)");
  return 0;
}

}  // namespace crnerf

using namespace crnerf;

extern "C" size_t crnerf_mesh_parts_workspace_bytes(int64_t V, int64_t F) {
  if (V <= 0 || F < 0 || V > MESH_MAX || F > MESH_MAX) return 0;
  return (size_t)8 * scan_blocks((uint32_t)V) + (size_t)8 * scan_blocks((uint32_t)F) + (size_t)6 * (size_t)V + (size_t)2 * (size_t)F + MP_WORKSPACE_PAD;
}

extern "C" int crnerf_mesh_parts_label_i32(const int32_t* faces, int64_t V, int64_t F, void* workspace, int32_t* vertex_part, int32_t* face_part,
                                           int64_t* counts, void* stream) {
  static const char* who = "mesh_parts_label";
  if (int rc = mesh_sizes(who, V, F)) return rc;
  hipStream_t st = (hipStream_t)stream;
  if (V == 0) {                                 // no vertex: K = 0, nothing is launched
    if (counts && hipMemsetAsync(counts, 0, sizeof(int64_t), st) != hipSuccess)
      return set_error(CRNERF_ERR_HIP, "mesh_parts_label: hipMemsetAsync(counts) failed");
    return 0;
  }
  MESH_REQUIRE(workspace, who, "workspace"); MESH_REQUIRE(vertex_part, who, "vertex_part"); MESH_REQUIRE(counts, who, "counts");
  if (F > 0) { MESH_REQUIRE(faces, who, "faces"); MESH_REQUIRE(face_part, who, "face_part"); }
  MESH_ALIGNED(workspace, who);
  const uint32_t v = (uint32_t)V, f = (uint32_t)F;
  const MpWorkspace w = mp_carve(workspace, v, f);
  if (int rc = mesh_launch(parts_init_kernel, "parts_init_kernel", launch_blocks(v, MESH_THREADS), MESH_THREADS, st, w.parent, v)) return rc;
  if (f > 0) {
    if (int rc = mesh_launch(parts_union_kernel, "parts_union_kernel", launch_blocks(f, MESH_THREADS), MESH_THREADS, st, faces, v, f, w.parent)) return rc;
  }
  if (int rc = mesh_launch(parts_roots_kernel, "parts_roots_kernel", scan_blocks(v), MESH_PER_THREADS, st, w.parent, v, w.vloc, w.vbase)) return rc;
  if (int rc = mesh_block_scan(st, ScanList<1>{w.vbase, scan_blocks(v), {(long long*)counts}})) return rc;
  return mesh_launch(parts_apply_kernel, "parts_apply_kernel", launch_blocks(v > f ? v : f, MESH_THREADS), MESH_THREADS, st, faces, v, f, w, vertex_part,
                     f > 0 ? face_part : (int32_t*)nullptr);
}

extern "C" int crnerf_mesh_parts_sizes_i32(const int32_t* vertex_part, const int32_t* face_part, int64_t V, int64_t F, int64_t K,
                                           int32_t* part_vertices, int32_t* part_faces, void* stream) {
  static const char* who = "mesh_parts_sizes";
  if (int rc = mesh_sizes(who, V, F)) return rc;
  if (int rc = mp_parts(who, V, K)) return rc;
  if (V == 0 || K == 0) return 0;
  MESH_REQUIRE(vertex_part, who, "vertex_part"); MESH_REQUIRE(part_vertices, who, "part_vertices"); MESH_REQUIRE(part_faces, who, "part_faces");
  if (F > 0) MESH_REQUIRE(face_part, who, "face_part");
  hipStream_t st = (hipStream_t)stream;
  MESH_FILL(part_vertices, 0, sizeof(int32_t) * (size_t)K, st, who);
  MESH_FILL(part_faces, 0, sizeof(int32_t) * (size_t)K, st, who);
  const uint32_t per = MESH_THREADS * MP_SIZE_STEPS;
  auto blocks = [per](uint32_t n) { const uint32_t b = launch_blocks(n, per); return b < (uint32_t)MP_SIZE_BLOCKS ? b : (uint32_t)MP_SIZE_BLOCKS; };
  if (int rc = mesh_launch(parts_sizes_kernel, "parts_sizes_kernel", blocks((uint32_t)V), MESH_THREADS, st, vertex_part, (uint32_t)V, (uint32_t)K, part_vertices))
    return rc;
  if (F > 0) return mesh_launch(parts_sizes_kernel, "parts_sizes_kernel", blocks((uint32_t)F), MESH_THREADS, st, face_part, (uint32_t)F, (uint32_t)K, part_faces);
  return 0;
}

extern "C" int crnerf_mesh_parts_select_count(const int32_t* vertex_part, const int32_t* face_part, int64_t V, int64_t F, int64_t K,
                                              const uint8_t* keep, void* workspace, int64_t* counts, void* stream) {
  static const char* who = "mesh_parts_select_count";
  if (int rc = mesh_sizes(who, V, F)) return rc;
  if (int rc = mp_parts(who, V, K)) return rc;
  hipStream_t st = (hipStream_t)stream;
  if (V == 0) {
    if (counts && hipMemsetAsync(counts, 0, 2 * sizeof(int64_t), st) != hipSuccess)
      return set_error(CRNERF_ERR_HIP, "mesh_parts_select_count: hipMemsetAsync(counts) failed");
    return 0;
  }
  MESH_REQUIRE(vertex_part, who, "vertex_part"); MESH_REQUIRE(workspace, who, "workspace"); MESH_REQUIRE(counts, who, "counts");
  if (F > 0) MESH_REQUIRE(face_part, who, "face_part");
  if (K > 0) MESH_REQUIRE(keep, who, "keep");
  MESH_ALIGNED(workspace, who);
  const uint32_t v = (uint32_t)V, f = (uint32_t)F;
  const MpWorkspace w = mp_carve(workspace, v, f);
  if (int rc = mesh_launch(parts_keep_kernel, "parts_keep_kernel", scan_blocks(v), MESH_PER_THREADS, st, vertex_part, v, (uint32_t)K, keep, w.vloc, w.vbase))
    return rc;
  if (f > 0) {
    if (int rc = mesh_launch(parts_keep_kernel, "parts_keep_kernel", scan_blocks(f), MESH_PER_THREADS, st, face_part, f, (uint32_t)K, keep, w.floc, w.fbase))
      return rc;
  }
  long long* const out = (long long*)counts;
  return mesh_block_scan(st, ScanList<1>{w.vbase, scan_blocks(v), {out}}, ScanList<1>{w.fbase, scan_blocks(f), {out + 1}});
}

extern "C" int crnerf_mesh_parts_select_emit_f32(const float* vertices, const float* normals, const int32_t* faces, const int32_t* vertex_part,
                                                 const int32_t* face_part, int64_t V, int64_t F, int64_t K, const uint8_t* keep,
                                                 const void* workspace, int64_t v_cap, int64_t f_cap, float* out_vertices, float* out_normals,
                                                 int32_t* out_faces, void* stream) {
  static const char* who = "mesh_parts_select_emit";
  if (int rc = mesh_sizes(who, V, F)) return rc;
  if (int rc = mp_parts(who, V, K)) return rc;
  if (int rc = mesh_caps(who, v_cap, f_cap)) return rc;
  const bool want_v = v_cap > 0, want_f = f_cap > 0 && F > 0;
  if (V == 0 || K == 0 || (!want_v && !want_f)) return 0;      // K == 0: nothing is kept
  MESH_REQUIRE(vertex_part, who, "vertex_part"); MESH_REQUIRE(keep, who, "keep"); MESH_REQUIRE(workspace, who, "workspace");
  if (want_v) {
    MESH_REQUIRE(vertices, who, "vertices"); MESH_REQUIRE(out_vertices, who, "out_vertices");
    if (normals) MESH_REQUIRE(out_normals, who, "out_normals");
  }
  if (want_f) { MESH_REQUIRE(faces, who, "faces"); MESH_REQUIRE(face_part, who, "face_part"); MESH_REQUIRE(out_faces, who, "out_faces"); }
  MESH_ALIGNED(workspace, who);
  const uint32_t v = (uint32_t)V, f = want_f ? (uint32_t)F : 0u;
  const MpWorkspace w = mp_carve(const_cast<void*>(workspace), v, (uint32_t)F);
  return mesh_launch(parts_emit_kernel, "parts_emit_kernel", launch_blocks(v > f ? v : f, MESH_THREADS), MESH_THREADS, (hipStream_t)stream,
                     (const uint32_t*)vertices, (const uint32_t*)normals, faces, vertex_part, face_part, v, f, (uint32_t)K, keep, w, (long long)v_cap,
                     (long long)f_cap, (uint32_t*)out_vertices, (uint32_t*)out_normals, out_faces);
}

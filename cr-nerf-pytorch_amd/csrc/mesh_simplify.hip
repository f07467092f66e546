// Mesh simplification by vertex clustering (csrc/crnerf_mesh_simplify.h carries every rule): one vertex per occupied cell of a
// grid, positions, normals and colours from exact integer sums, the faces remapped, the collapsed and the duplicate ones dropped -- the same bytes
// on every run.
//
// Count, nine launches (six when F = 0) behind two fills, none of which waits on another workgroup:
//   (fill)                    leader[cells] = 0xffffffff, table[T] = -1
//   cluster_key_kernel        one thread per vertex: key[v] = its cell; atomicMin(leader[key], v) -- by the first lane of every run of equal keys in
//                             a wave only: the lanes of a wave hold rising ids, so that lane holds the run's smallest
//   cluster_leaders_kernel    flag[v] = leader[key[v]] == v; the block scan of mesh_common.h over the flags
//   mesh_block_scan_kernel    (mesh_common.h) the vertices' block totals: counts[0] and, kept for emit, totals[0]
//   cluster_apply_kernel      vertex_cluster[v] = base[block(leader)] + rank[leader]; the leader writes ckey[cluster] = key
//   cluster_faces_kernel      one thread per face: an invalid face is dropped before any of its ids is used; tri[f] = its three cluster ids,
//                             sorted; tri[f][0] = -1 for an invalid or a collapsed face
//   cluster_insert_kernel     the survivors into table[T] (T: the smallest power of two >= 2 F), linear probing from a hash of the sorted triple:
//                             an empty slot is claimed by CAS, a slot that holds a face of the same set takes atomicMin(slot, f), any other slot is
//                             passed.  A slot never empties and only ever changes to a face of the SAME set, so every face of a set stops at the
//                             set's one slot, and that slot ends as the set's smallest face index whatever order the inserts ran in.  fslot[f] =
//                             the slot.  The triples compared were written by the launch before: plain reads
//   cluster_keep_kernel       kept[f] = survivor && table[fslot[f]] == f; block scan, rank and flag in floc[f]
//   mesh_block_scan_kernel    again, over the faces' block totals: counts[1], totals[1]
// Emit: (fill) the sums of the clusters below v_cap = 0; cluster_sum_kernel (integer atomicAdd on 64-bit words: exact, so deterministic; the
// lanes of a run of equal clusters are merged first, mesh_common.h, and the run's last lane adds -- adds to one address retire one after
// another, about 26 ns each (profiles/r22/mesh_parts.txt), and the ids of an extracted mesh are spatially coherent); cluster_finish_kernel, one
// thread per cluster; cluster_emit_faces_kernel.
//
// Coherence.  The XCDs' L2s are not coherent for plain accesses inside one kernel (mesh_parts.hip): leader[] and table[] are touched with
// agent-scope atomics only -- loads included -- inside the kernels that write them, and the sums by atomic adds only; later launches read all
// three plainly.
//
// Workspace: totals[2] (int64: V', F') | vbase[nbV] fbase[nbF] (uint64) | leader[cells] (uint32) | key[V] (int32) | vloc[V] | floc[F] (uint16) | tri[F][3] (int32) |
// fslot[F] (uint32) | table[T] (int32) | ckey[C] (int32) | sums[C][10] (int64), C = min(V, cells); every array on a 16-byte boundary.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include "crnerf_mesh_simplify.h"
#include "mesh_common.h"

namespace crnerf {

constexpr int32_t MS_MAX_AXIS = 1 << 20;
constexpr int MS_SUMS = 10;                     // per cluster: 3 position sums, the member count, 3 normal sums, 3 colour sums
constexpr uint16_t MS_KEPT = 0x8000;            // floc[f]: the rank inside the block (< 1,024) and this flag
constexpr float MS_FIXED = 1048576.0f;          // 2^20
static_assert(MESH_SCAN <= MS_KEPT, "a rank inside a block and the kept flag share 16 bits");

struct MsGrid {
  float lo[3], inv[3], cell[3];
  int32_t n[3];
};

struct MsWorkspace {
  long long* totals;              // [2] V', F': what count wrote to counts[], kept for emit
  unsigned long long* vbase;      // [nbV] block totals, then exclusive bases
  unsigned long long* fbase;      // [nbF]
  uint32_t* leader;               // [cells] smallest member id, 0xffffffff: empty
  int32_t* key;                   // [V]
  uint16_t* vloc;                 // [V] leaders of the block below this one
  uint16_t* floc;                 // [F] kept faces of the block below this one | MS_KEPT
  int32_t* tri;                   // [F][3] sorted cluster ids; [0] = -1: dropped
  uint32_t* fslot;                // [F]
  int32_t* table;                 // [T] face indices, -1: empty
  int32_t* ckey;                  // [C] cell key of a cluster
  long long* sums;                // [C][MS_SUMS]
  uint64_t slots;                 // T
};

constexpr size_t MS_WORKSPACE_PAD = 192;        // totals[2], and eleven roundings of at most 15 bytes each

static uint64_t ms_slots(uint32_t F) {          // the smallest power of two >= 2 F (F > 0), at most 2^32
  uint64_t t = 1;
  while (t < 2 * (uint64_t)F) t <<= 1;
  return t;
}
static inline uint64_t ms_clusters(uint32_t V, uint64_t cells) { return V < cells ? V : cells; }

static MsWorkspace ms_carve(void* workspace, uint32_t V, uint32_t F, uint64_t cells) {
  MsWorkspace w;
  char* p = (char*)workspace;
  size_t off = 0;
  const uint64_t C = ms_clusters(V, cells);
  w.slots = F ? ms_slots(F) : 0;
  w.totals = (long long*)(p + off); off += 16;
  w.vbase = (unsigned long long*)(p + off); off = align16(off + 8 * (size_t)scan_blocks(V));
  w.fbase = (unsigned long long*)(p + off); off = align16(off + 8 * (size_t)scan_blocks(F));
  w.leader = (uint32_t*)(p + off); off = align16(off + 4 * (size_t)cells);
  w.key = (int32_t*)(p + off); off = align16(off + 4 * (size_t)V);
  w.vloc = (uint16_t*)(p + off); off = align16(off + 2 * (size_t)V);
  w.floc = (uint16_t*)(p + off); off = align16(off + 2 * (size_t)F);
  w.tri = (int32_t*)(p + off); off = align16(off + 12 * (size_t)F);
  w.fslot = (uint32_t*)(p + off); off = align16(off + 4 * (size_t)F);
  w.table = (int32_t*)(p + off); off = align16(off + 4 * (size_t)w.slots);
  w.ckey = (int32_t*)(p + off); off = align16(off + 4 * (size_t)C);
  w.sums = (long long*)(p + off);
  return w;
}

// ---------------------------------------------------------------------------------------------------------------- the cell of a vertex
// s (clamped to [0, n]) and c = min((int) s, n - 1) of one coordinate.  A NaN is found in the bits -- the unit is built with -fno-honor-nans -- and
// the integer is clamped after the conversion: c lies in [0, n) whatever v was.
__device__ __forceinline__ int32_t ms_cell(float v, float lo, float inv, int32_t n, float& s_out) {
  float s = (v - lo) * inv;
  if ((__float_as_uint(s) & 0x7fffffffu) > 0x7f800000u) s = 0.0f;
  s = fminf(fmaxf(s, 0.0f), (float)n);
  int32_t c = (int32_t)s;
  c = c < n - 1 ? c : n - 1;
  c = c > 0 ? c : 0;
  s_out = s;
  return c;
}

// r = (int) floorf((s - (float) c) * 2^20), clamped to [0, 2^20] after the conversion
__device__ __forceinline__ int32_t ms_fraction(float s, int32_t c) {
  int32_t r = (int32_t)floorf((s - (float)c) * MS_FIXED);
  r = r < (1 << 20) ? r : (1 << 20);
  return r > 0 ? r : 0;
}

// q = (int) rintf(clamp(x, lo, hi) * 2^20), clamped again after the conversion
__device__ __forceinline__ int32_t ms_fixed(float x, float lo, float hi) {
  if ((__float_as_uint(x) & 0x7fffffffu) > 0x7f800000u) x = 0.0f;
  int32_t q = (int32_t)rintf(fminf(fmaxf(x, lo), hi) * MS_FIXED);
  const int32_t qlo = (int32_t)(lo * MS_FIXED), qhi = (int32_t)(hi * MS_FIXED);
  q = q < qhi ? q : qhi;
  return q > qlo ? q : qlo;
}

__global__ __launch_bounds__(MESH_THREADS) void cluster_key_kernel(const float* __restrict__ vertices, uint32_t V, MsGrid g, int32_t* __restrict__ key,
                                                                 uint32_t* leader) {
  const uint32_t v = blockIdx.x * (uint32_t)MESH_THREADS + threadIdx.x, lane = threadIdx.x & 63;
  int32_t k = -1;                                            // (past the end: a run of its own that adds nothing)
  if (v < V) {
    float s;
    const int32_t c0 = ms_cell(vertices[3 * (size_t)v], g.lo[0], g.inv[0], g.n[0], s);
    const int32_t c1 = ms_cell(vertices[3 * (size_t)v + 1], g.lo[1], g.inv[1], g.n[1], s);
    const int32_t c2 = ms_cell(vertices[3 * (size_t)v + 2], g.lo[2], g.inv[2], g.n[2], s);
    k = c0 + g.n[0] * (c1 + g.n[1] * c2);                    // < n0 n1 n2 <= 2^31 - 1
    key[v] = k;
  }
  unsigned long long heads;
  const uint32_t first = run_first(k, lane, heads);
  if (v < V && first == lane) atomicMin(leader + k, v);
}

// ---------------------------------------------------------------------------------------------------------------- flags -> offsets inside a block
__global__ __launch_bounds__(MESH_PER_THREADS) void cluster_leaders_kernel(const int32_t* __restrict__ key, const uint32_t* __restrict__ leader, uint32_t V,
                                                                          uint16_t* __restrict__ loc, unsigned long long* __restrict__ base) {
  const uint32_t i0 = blockIdx.x * (uint32_t)MESH_SCAN + MESH_PER * threadIdx.x;
  uint32_t flag[MESH_PER];
#pragma unroll
  for (int j = 0; j < MESH_PER; ++j) flag[j] = (i0 + j < V && leader[key[i0 + j]] == i0 + j) ? 1u : 0u;
  block_offsets(flag, i0, V, 0, loc, base);
}

__global__ __launch_bounds__(MESH_PER_THREADS) void cluster_keep_kernel(const int32_t* __restrict__ tri, const uint32_t* __restrict__ fslot,
                                                                       const int32_t* __restrict__ table, uint32_t F, uint16_t* __restrict__ loc,
                                                                       unsigned long long* __restrict__ base) {
  const uint32_t i0 = blockIdx.x * (uint32_t)MESH_SCAN + MESH_PER * threadIdx.x;
  uint32_t flag[MESH_PER];
#pragma unroll
  for (int j = 0; j < MESH_PER; ++j) {
    const uint32_t f = i0 + j;
    flag[j] = (f < F && tri[3 * (size_t)f] >= 0 && table[fslot[f]] == (int32_t)f) ? 1u : 0u;
  }
  block_offsets(flag, i0, F, MS_KEPT, loc, base);
}

// ---------------------------------------------------------------------------------------------------------------- cluster ids
__global__ __launch_bounds__(MESH_THREADS) void cluster_apply_kernel(uint32_t V, MsWorkspace w, int32_t* __restrict__ vertex_cluster) {
  const uint32_t v = blockIdx.x * (uint32_t)MESH_THREADS + threadIdx.x;
  if (v >= V) return;
  const int32_t k = w.key[v];
  const uint32_t l = w.leader[k];                            // <= v < V: some member lowered it
  const int32_t id = (int32_t)(w.vbase[l >> MESH_SCAN_SHIFT] + w.vloc[l]);
  vertex_cluster[v] = id;
  if (l == v) w.ckey[id] = k;                                // id < the number of occupied cells <= min(V, cells)
}

// ---------------------------------------------------------------------------------------------------------------- faces
__global__ __launch_bounds__(MESH_THREADS) void cluster_faces_kernel(const int32_t* __restrict__ faces, const int32_t* __restrict__ vertex_cluster,
                                                                   uint32_t V, uint32_t F, int32_t* __restrict__ tri) {
  const uint32_t f = blockIdx.x * (uint32_t)MESH_THREADS + threadIdx.x;
  if (f >= F) return;                                        // (tested here as well: a dropped face below F still gets its tri[f])
  int32_t id[3], x = -1, y = -1, z = -1;
  if (load_face(faces, f, F, V, id)) {
    x = vertex_cluster[id[0]]; y = vertex_cluster[id[1]]; z = vertex_cluster[id[2]];
    if (x == y || x == z || y == z) {
      x = y = z = -1;
    } else {
      if (x > y) { const int32_t t = x; x = y; y = t; }
      if (y > z) { const int32_t t = y; y = z; z = t; }
      if (x > y) { const int32_t t = x; x = y; y = t; }
    }
  }
  tri[3 * (size_t)f] = x; tri[3 * (size_t)f + 1] = y; tri[3 * (size_t)f + 2] = z;
}

__device__ __forceinline__ uint32_t ms_hash(uint32_t x, uint32_t y, uint32_t z) {
  uint32_t h = x * 0x9e3779b1u;
  h = (h << 13 | h >> 19) + y * 0x85ebca77u;
  h = (h << 13 | h >> 19) + z * 0xc2b2ae3du;
  h ^= h >> 16; h *= 0x85ebca6bu; h ^= h >> 13; h *= 0xc2b2ae35u; h ^= h >> 16;      // (the low bits pick the slot)
  return h;
}

__global__ __launch_bounds__(MESH_THREADS) void cluster_insert_kernel(const int32_t* __restrict__ tri, uint32_t F, uint32_t mask, int32_t* table,
                                                                    uint32_t* __restrict__ fslot) {
  const uint32_t f = blockIdx.x * (uint32_t)MESH_THREADS + threadIdx.x;
  if (f >= F) return;
  const int32_t x = tri[3 * (size_t)f], y = tri[3 * (size_t)f + 1], z = tri[3 * (size_t)f + 2];
  if (x < 0) return;
  uint32_t slot = ms_hash((uint32_t)x, (uint32_t)y, (uint32_t)z) & mask;
  // at most F of the >= 2 F slots are ever taken, so an empty slot or the set's own is met before the walk comes round
  for (;;) {
    int32_t held = __hip_atomic_load(table + slot, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (held < 0) {
      held = atomicCAS(table + slot, -1, (int32_t)f);
      if (held < 0) break;                                   // claimed
    }
    // held: a face index in [0, F) -- the table holds nothing else --, a survivor, so its triple is three cluster ids
    if (tri[3 * (size_t)held] == x && tri[3 * (size_t)held + 1] == y && tri[3 * (size_t)held + 2] == z) {
      if ((int32_t)f < held) atomicMin(table + slot, (int32_t)f);
      break;
    }
    slot = (slot + 1) & mask;
  }
  fslot[f] = slot;
}

// ---------------------------------------------------------------------------------------------------------------- emit
__device__ __forceinline__ void ms_add(long long* p, int32_t x) { atomicAdd((unsigned long long*)p, (unsigned long long)(long long)x); }

__global__ __launch_bounds__(MESH_THREADS) void cluster_sum_kernel(const float* __restrict__ vertices, const float* __restrict__ normals,
                                                                 const float* __restrict__ colors, const int32_t* __restrict__ vertex_cluster,
                                                                 uint32_t V, MsGrid g, long long v_cap, long long* sums) {
  const uint32_t v = blockIdx.x * (uint32_t)MESH_THREADS + threadIdx.x, lane = threadIdx.x & 63;
  int32_t id = -1, r[3] = {0, 0, 0}, qn[3] = {0, 0, 0}, qc[3] = {0, 0, 0};
  if (v < V) {
    id = vertex_cluster[v];
    if (id < 0 || id >= v_cap) id = -1;                      // (a cluster whose row is not written needs no sums)
  }
  if (id >= 0) {
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      float s;
      const int32_t c = ms_cell(vertices[3 * (size_t)v + a], g.lo[a], g.inv[a], g.n[a], s);
      r[a] = ms_fraction(s, c);
      if (normals) qn[a] = ms_fixed(normals[3 * (size_t)v + a], -1.0f, 1.0f);
      if (colors) qc[a] = ms_fixed(colors[3 * (size_t)v + a], 0.0f, 1.0f);
    }
  }
  // a run is at most 64 lanes long: its sums stay below 2^27 in magnitude
  unsigned long long heads;
  const uint32_t first = run_first(id, lane, heads);
  const bool last = run_last(heads, lane);
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    r[a] = run_sum(r[a], lane, first);
    if (normals) qn[a] = run_sum(qn[a], lane, first);        // (normals, colors: the same in every lane)
    if (colors) qc[a] = run_sum(qc[a], lane, first);
  }
  if (id < 0 || !last) return;
  long long* p = sums + (size_t)MS_SUMS * (size_t)id;
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    ms_add(p + a, r[a]);
    if (normals) ms_add(p + 4 + a, qn[a]);
    if (colors) ms_add(p + 7 + a, qc[a]);
  }
  ms_add(p + 3, (int32_t)(lane - first + 1));
}

__global__ __launch_bounds__(MESH_THREADS) void cluster_finish_kernel(const long long* __restrict__ totals, const int32_t* __restrict__ ckey,
                                                                    const long long* __restrict__ sums, MsGrid g, long long v_cap, int has_normals,
                                                                    int has_colors, float* __restrict__ out_vertices, float* __restrict__ out_normals,
                                                                    float* __restrict__ out_colors) {
  const long long id = (long long)blockIdx.x * MESH_THREADS + threadIdx.x;
  if (id >= v_cap || id >= totals[0]) return;                // (a row past V' is not written either)
  const long long* p = sums + (size_t)MS_SUMS * (size_t)id;
  int32_t k = ckey[id];
  int32_t c[3];
  c[0] = k % g.n[0]; k /= g.n[0];
  c[1] = k % g.n[1];
  c[2] = k / g.n[1];
  const double scale = (double)p[3] * 1048576.0;
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    const double t = (double)c[a] + (double)p[a] / scale;
    out_vertices[3 * id + a] = (float)((double)g.lo[a] + t * (double)g.cell[a]);
  }
  if (has_normals) {
    const double x = (double)p[4], y = (double)p[5], z = (double)p[6];
    const bool zero = p[4] == 0 && p[5] == 0 && p[6] == 0;
    const double d = sqrt(x * x + y * y + z * z);
    out_normals[3 * id] = zero ? 0.0f : (float)(x / d);
    out_normals[3 * id + 1] = zero ? 0.0f : (float)(y / d);
    out_normals[3 * id + 2] = zero ? 0.0f : (float)(z / d);
  }
  if (has_colors) {
#pragma unroll
    for (int a = 0; a < 3; ++a) out_colors[3 * id + a] = (float)((double)p[7 + a] / scale);
  }
}

__global__ __launch_bounds__(MESH_THREADS) void cluster_emit_faces_kernel(const int32_t* __restrict__ faces, const int32_t* __restrict__ vertex_cluster,
                                                                        uint32_t V, uint32_t F, const uint16_t* __restrict__ floc,
                                                                        const unsigned long long* __restrict__ fbase, long long f_cap,
                                                                        int32_t* __restrict__ out_faces) {
  const uint32_t f = blockIdx.x * (uint32_t)MESH_THREADS + threadIdx.x;
  if (f >= F) return;
  const uint16_t loc = floc[f];
  if (!(loc & MS_KEPT)) return;
  const long long id = (long long)(fbase[f >> MESH_SCAN_SHIFT] + (loc & (MS_KEPT - 1)));
  if (id >= f_cap) return;
  // kept: the ids passed the test of cluster_faces_kernel; they are tested again -- emit may be handed other faces than count was
  int32_t id3[3];
  if (!load_face(faces, f, F, V, id3)) return;
  const int32_t a = vertex_cluster[id3[0]], b = vertex_cluster[id3[1]], c = vertex_cluster[id3[2]];
  int32_t x = a, y = b, z = c;                               // the cycle as given, the smallest id first
  if (b < a && b < c) { x = b; y = c; z = a; }
  else if (c < a && c < b) { x = c; y = a; z = b; }
  out_faces[3 * id] = x; out_faces[3 * id + 1] = y; out_faces[3 * id + 2] = z;
}

// ---------------------------------------------------------------------------------------------------------------- host
// the nine scalars, judged and folded into an MsGrid; *cells = n0 n1 n2
static int ms_grid_of(const char* who, const float lo[3], const float cell[3], const int32_t n[3], MsGrid* g, uint64_t* cells) {
  uint64_t total = 1;
  for (int a = 0; a < 3; ++a) {
    if (n[a] < 1) return launch_fail(CRNERF_ERR_SHAPE, who, "fewer than one cell on an axis");
    if (n[a] > MS_MAX_AXIS) return launch_fail(CRNERF_ERR_SHAPE, who, "more than 2^20 cells on an axis");
    total *= (uint64_t)n[a];                                 // <= 2^60
  }
  if (total > (uint64_t)MESH_MAX) return launch_fail(CRNERF_ERR_SHAPE, who, "more than 2^31 - 1 cells");
  for (int a = 0; a < 3; ++a) {
    if (!std::isfinite(cell[a]) || !(cell[a] > 0.0f)) return launch_fail(CRNERF_ERR_SHAPE, who, "a cell size that is not finite and > 0");
    const float inv = 1.0f / cell[a];
    if (!std::isfinite(inv)) return launch_fail(CRNERF_ERR_SHAPE, who, "a cell size whose float32 reciprocal is not finite");
    if (!std::isfinite(lo[a])) return launch_fail(CRNERF_ERR_SHAPE, who, "a box origin that is not finite");
    g->lo[a] = lo[a]; g->inv[a] = inv; g->cell[a] = cell[a]; g->n[a] = n[a];
  }
  *cells = total;
  return 0;
}

}  // namespace crnerf

using namespace crnerf;

extern "C" size_t crnerf_mesh_cluster_workspace_bytes(int64_t V, int64_t F, int64_t cells) {
  if (V <= 0 || F < 0 || V > MESH_MAX || F > MESH_MAX || cells < 1 || cells > MESH_MAX) return 0;
  const uint32_t v = (uint32_t)V, f = (uint32_t)F;
  return (size_t)8 * scan_blocks(v) + (size_t)8 * scan_blocks(f) + (size_t)4 * (size_t)cells + (size_t)6 * (size_t)V + (size_t)18 * (size_t)F +
         (size_t)4 * (size_t)(f ? ms_slots(f) : 0) + (size_t)(4 + 8 * MS_SUMS) * (size_t)ms_clusters(v, (uint64_t)cells) + MS_WORKSPACE_PAD;
}

extern "C" int crnerf_mesh_cluster_count_f32(const float* vertices, const int32_t* faces, int64_t V, int64_t F, float lo0, float lo1, float lo2,
                                             float cell0, float cell1, float cell2, int32_t n0, int32_t n1, int32_t n2, void* workspace,
                                             int32_t* vertex_cluster, int64_t* counts, void* stream) {
  static const char* who = "mesh_cluster_count";
  if (int rc = mesh_sizes(who, V, F)) return rc;
  MsGrid g;
  uint64_t cells;
  const float lo[3] = {lo0, lo1, lo2}, cell[3] = {cell0, cell1, cell2};
  const int32_t n[3] = {n0, n1, n2};
  if (int rc = ms_grid_of(who, lo, cell, n, &g, &cells)) return rc;
  hipStream_t st = (hipStream_t)stream;
  if (V == 0) {                                 // no vertex: V' = F' = 0, nothing is launched
    if (counts) MESH_FILL(counts, 0, 2 * sizeof(int64_t), st, who);
    return 0;
  }
  MESH_REQUIRE(vertices, who, "vertices"); MESH_REQUIRE(workspace, who, "workspace"); MESH_REQUIRE(vertex_cluster, who, "vertex_cluster");
  MESH_REQUIRE(counts, who, "counts");
  if (F > 0) MESH_REQUIRE(faces, who, "faces");
  MESH_ALIGNED(workspace, who);
  const uint32_t v = (uint32_t)V, f = (uint32_t)F;
  const MsWorkspace w = ms_carve(workspace, v, f, cells);
  const uint32_t vblocks = launch_blocks(v, MESH_THREADS), fblocks = launch_blocks(f, MESH_THREADS);
  long long* const out = (long long*)counts;
  MESH_FILL(w.leader, 0xff, 4 * (size_t)cells, st, who);
  if (int rc = mesh_launch(cluster_key_kernel, "cluster_key_kernel", vblocks, MESH_THREADS, st, vertices, v, g, w.key, w.leader)) return rc;
  if (int rc = mesh_launch(cluster_leaders_kernel, "cluster_leaders_kernel", scan_blocks(v), MESH_PER_THREADS, st, w.key, w.leader, v, w.vloc, w.vbase))
    return rc;
  if (int rc = mesh_block_scan(st, ScanList<2>{w.vbase, scan_blocks(v), {out, w.totals}})) return rc;
  if (int rc = mesh_launch(cluster_apply_kernel, "cluster_apply_kernel", vblocks, MESH_THREADS, st, v, w, vertex_cluster)) return rc;
  if (f > 0) {
    MESH_FILL(w.table, 0xff, 4 * (size_t)w.slots, st, who);
    if (int rc = mesh_launch(cluster_faces_kernel, "cluster_faces_kernel", fblocks, MESH_THREADS, st, faces, vertex_cluster, v, f, w.tri)) return rc;
    if (int rc = mesh_launch(cluster_insert_kernel, "cluster_insert_kernel", fblocks, MESH_THREADS, st, w.tri, f, (uint32_t)(w.slots - 1), w.table, w.fslot))
      return rc;
    if (int rc = mesh_launch(cluster_keep_kernel, "cluster_keep_kernel", scan_blocks(f), MESH_PER_THREADS, st, w.tri, w.fslot, w.table, f, w.floc, w.fbase))
      return rc;
  }
  return mesh_block_scan(st, ScanList<2>{w.fbase, scan_blocks(f), {out + 1, w.totals + 1}});      // (F = 0: no block, the sum is 0)
}

extern "C" int crnerf_mesh_cluster_emit_f32(const float* vertices, const float* normals, const float* colors, const int32_t* faces,
                                            const int32_t* vertex_cluster, int64_t V, int64_t F, float lo0, float lo1, float lo2, float cell0,
                                            float cell1, float cell2, int32_t n0, int32_t n1, int32_t n2, void* workspace, int64_t v_cap,
                                            int64_t f_cap, float* out_vertices, float* out_normals, float* out_colors, int32_t* out_faces,
                                            void* stream) {
  static const char* who = "mesh_cluster_emit";
  if (int rc = mesh_sizes(who, V, F)) return rc;
  if (int rc = mesh_caps(who, v_cap, f_cap)) return rc;
  MsGrid g;
  uint64_t cells;
  const float lo[3] = {lo0, lo1, lo2}, cell[3] = {cell0, cell1, cell2};
  const int32_t n[3] = {n0, n1, n2};
  if (int rc = ms_grid_of(who, lo, cell, n, &g, &cells)) return rc;
  const bool want_v = v_cap > 0, want_f = f_cap > 0 && F > 0;
  if (V == 0 || (!want_v && !want_f)) return 0;
  MESH_REQUIRE(vertex_cluster, who, "vertex_cluster"); MESH_REQUIRE(workspace, who, "workspace");
  if (want_v) {
    MESH_REQUIRE(vertices, who, "vertices"); MESH_REQUIRE(out_vertices, who, "out_vertices");
    if (normals) MESH_REQUIRE(out_normals, who, "out_normals");
    if (colors) MESH_REQUIRE(out_colors, who, "out_colors");
  }
  if (want_f) { MESH_REQUIRE(faces, who, "faces"); MESH_REQUIRE(out_faces, who, "out_faces"); }
  MESH_ALIGNED(workspace, who);
  hipStream_t st = (hipStream_t)stream;
  const uint32_t v = (uint32_t)V, f = (uint32_t)F;
  const MsWorkspace w = ms_carve(workspace, v, f, cells);
  if (want_v) {
    const uint64_t C = ms_clusters(v, cells), rows = (uint64_t)v_cap < C ? (uint64_t)v_cap : C;      // V' <= C: no cluster id reaches C
    MESH_FILL(w.sums, 0, sizeof(long long) * MS_SUMS * (size_t)rows, st, who);
    if (int rc = mesh_launch(cluster_sum_kernel, "cluster_sum_kernel", launch_blocks(v, MESH_THREADS), MESH_THREADS, st, vertices, normals, colors,
                             vertex_cluster, v, g, (long long)rows, w.sums))
      return rc;
    if (int rc = mesh_launch(cluster_finish_kernel, "cluster_finish_kernel", launch_blocks(rows, MESH_THREADS), MESH_THREADS, st, w.totals, w.ckey, w.sums, g,
                             (long long)rows, normals ? 1 : 0, colors ? 1 : 0, out_vertices, out_normals, out_colors))
      return rc;
  }
  if (want_f)
    return mesh_launch(cluster_emit_faces_kernel, "cluster_emit_faces_kernel", launch_blocks(f, MESH_THREADS), MESH_THREADS, st, faces, vertex_cluster, v, f,
                       w.floc, w.fbase, (long long)f_cap, out_faces);
  return 0;
}

// Iso-surface extraction (include/crnerf_mesh.h carries every rule): marching tetrahedra on the Kuhn split of a
// [nz][ny][nx] float32 density grid -> an indexed triangle mesh (shared vertices, int32 faces, per-vertex normals), the same bytes on
// every run.
//
// Three launches, none of which waits on another workgroup:
//   mesh_count_kernel   one thread per 4 consecutive nodes: each node's 2x2x2 neighbourhood -> its 7-bit active-edge mask, its vertex count (the
//                       mask's popcount) and, where the node is a cell's origin, the cell's face count; the block scan of mesh_common.h over both
//                       counts at once (packed 16 + 16 bits: a block holds at most 7,168 vertices and 12,288 faces)
//   mesh_block_scan_kernel  (mesh_common.h) both lists of block totals: counts[0] = V, counts[1] = F
//   mesh_emit_kernel    one 16-byte load per 16 consecutive nodes' masks; a wave queues the active nodes of its 1,024 in LDS and walks them
//                       one per lane.  An active node writes its vertices at base[block] + local + rank and, as a cell's origin, its faces; a neighbour's vertex id is
//                       base[block(q)] + local[q] + popcount(mask[q] & ((1 << d) - 1)) -- the corner's inside bit is inside(origin) ^ mask bit,
//                       so no sigma is read twice for the topology.
// Offsets come from the scans alone: no atomics, so the order is the one the header defines.
//
// Workspace (5 bytes a node + 16 a block): vbase[nb] fbase[nb] (uint64) | mask[N] (uint8) | vloc[N] | floc[N] (uint16), nb = ceil(N / MESH_SCAN),
// every array on a 16-byte boundary.
// The passes are not bound by bytes (profiles/r21/mesh.txt): with one node per thread the count pass ran at 0.12 and the emit pass at 0.03-0.05 of
// their byte-count time, and staging the count pass's neighbourhoods through LDS changed its time by +2 % .. -7 %.  So the neighbourhoods overlap
// through L1 / L2, and the work per node was cut instead: four nodes share one index split, 20 independent loads instead of 32 branched ones and
// three stores instead of twelve; sixteen nodes share one mask load, and a wave's active nodes are walked one per lane.
//
// The unit is compiled with -fhonor-nans (build.py): `sigma > threshold` must be false for a NaN and `t >= 0 && t <= 1` false for a
// non-finite t.  The interpolation is written with __fmul_rn / __fadd_rn: a multiply and an add, rounded separately.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/crnerf_mesh.h"
#include "mesh_common.h"

namespace crnerf {

constexpr int MT_EMIT_THREADS = 256;
static_assert(7 * MESH_SCAN < 65536 && 12 * MESH_SCAN < 65536, "a block's vertex and face counts are scanned in 16 bits each");

// ---------------------------------------------------------------------------------------------------------------- the case table
// Tet t of a cell is the monotone path 0 -> 1 << a -> (1 << a) | (1 << b) -> 7 through the cell's corners (corner k = dx + 2 dy + 4 dz), (a, b, c)
// the t-th permutation of xyz in lexicographic order.  For each of the 16 inside patterns of its four nodes (bit j = path node j): the cycle
// of active edges, each as (lower corner, upper corner), oriented so that (v1 - v0) x (v2 - v0) points from the inside nodes to the outside
// ones.  Derived here, at compile time, on the unit cube with every vertex at its edge's midpoint (coordinates doubled: integers).
struct MtCase {
  unsigned char n;          // 0, 3 or 4 vertices
  unsigned char lo[4];      // edge j: corner lo[j] -> corner hi[j]; owner node = origin + lo, direction index = (hi - lo) - 1
  unsigned char hi[4];
};
struct MtTable { MtCase c[6][16]; };

constexpr int MT_AXES[6][3] = {{0, 1, 2}, {0, 2, 1}, {1, 0, 2}, {1, 2, 0}, {2, 0, 1}, {2, 1, 0}};

constexpr MtTable mt_make_table() {
  MtTable T{};
  for (int t = 0; t < 6; ++t) {
    const int corner[4] = {0, 1 << MT_AXES[t][0], (1 << MT_AXES[t][0]) | (1 << MT_AXES[t][1]), 7};
    for (int pat = 1; pat < 15; ++pat) {
      int I[4] = {0, 0, 0, 0}, O[4] = {0, 0, 0, 0}, nI = 0, nO = 0;
      for (int j = 0; j < 4; ++j) {
        if ((pat >> j) & 1) I[nI++] = j; else O[nO++] = j;
      }
      int ei[4] = {0, 0, 0, 0}, eo[4] = {0, 0, 0, 0}, n = 3;            // edge j joins path nodes ei[j] (inside) and eo[j] (outside)
      if (nI == 1) { for (int j = 0; j < 3; ++j) { ei[j] = I[0]; eo[j] = O[j]; } }
      else if (nO == 1) { for (int j = 0; j < 3; ++j) { ei[j] = I[j]; eo[j] = O[0]; } }
      else { n = 4; ei[0] = I[0]; eo[0] = O[0]; ei[1] = I[0]; eo[1] = O[1]; ei[2] = I[1]; eo[2] = O[1]; ei[3] = I[1]; eo[3] = O[0]; }
      int P[4][3] = {};                                                  // twice the edge midpoints
      for (int j = 0; j < n; ++j)
        for (int a = 0; a < 3; ++a) P[j][a] = ((corner[ei[j]] >> a) & 1) + ((corner[eo[j]] >> a) & 1);
      int nrm[3] = {0, 0, 0};
      for (int k = 1; k + 1 < n; ++k) {                                  // (P1 - P0) x (P2 - P0) [+ (P2 - P0) x (P3 - P0)]
        int u[3] = {}, v[3] = {};
        for (int a = 0; a < 3; ++a) { u[a] = P[k][a] - P[0][a]; v[a] = P[k + 1][a] - P[0][a]; }
        nrm[0] += u[1] * v[2] - u[2] * v[1]; nrm[1] += u[2] * v[0] - u[0] * v[2]; nrm[2] += u[0] * v[1] - u[1] * v[0];
      }
      int dot = 0;                                                       // nI nO (mean(outside) - mean(inside)) . nrm
      for (int a = 0; a < 3; ++a) {
        int sI = 0, sO = 0;
        for (int j = 0; j < nI; ++j) sI += (corner[I[j]] >> a) & 1;
        for (int j = 0; j < nO; ++j) sO += (corner[O[j]] >> a) & 1;
        dot += (nI * sO - nO * sI) * nrm[a];
      }
      MtCase& c = T.c[t][pat];
      c.n = (unsigned char)n;
      for (int j = 0; j < n; ++j) {
        const int s = dot < 0 ? n - 1 - j : j;
        const int p = ei[s] < eo[s] ? ei[s] : eo[s], q = ei[s] < eo[s] ? eo[s] : ei[s];      // path order is inclusion order
        c.lo[j] = (unsigned char)corner[p];
        c.hi[j] = (unsigned char)corner[q];
      }
    }
  }
  return T;
}

__constant__ const MtTable MT_TABLE = mt_make_table();
static_assert(mt_make_table().c[0][0].n == 0 && mt_make_table().c[5][15].n == 0 && mt_make_table().c[0][1].n == 3 && mt_make_table().c[3][6].n == 4,
              "no face without a sign change, a triangle for one inside node, a quad for two");

// ---------------------------------------------------------------------------------------------------------------- workspace
struct MtWorkspace {
  unsigned long long* vbase;      // [nb] the block's vertex total after the count pass, its exclusive base after the scan
  unsigned long long* fbase;      // [nb] the same for faces
  uint8_t* mask;                  // [N] bit d: the edge to p + direction d is active
  uint16_t* vloc;                 // [N] vertices of the block's nodes below this one
  uint16_t* floc;                 // [N] faces of the block's cells below this one
};

// every array starts on a 16-byte boundary of a 16-byte aligned workspace: the passes move 4 or 16 nodes' entries per load / store
constexpr size_t MT_WORKSPACE_PAD = 32;         // the two roundings, at most 15 bytes each

static MtWorkspace mt_carve(void* workspace, uint32_t N) {
  const size_t nb = scan_blocks(N);
  MtWorkspace w;
  char* p = (char*)workspace;
  size_t off = 0;
  w.vbase = (unsigned long long*)(p + off); off += 8 * nb;
  w.fbase = (unsigned long long*)(p + off); off += 8 * nb;
  w.mask = (uint8_t*)(p + off); off = align16(off + N);
  w.vloc = (uint16_t*)(p + off); off = align16(off + 2 * (size_t)N);
  w.floc = (uint16_t*)(p + off);
  return w;
}

// ---------------------------------------------------------------------------------------------------------------- count
// One thread per MESH_PER consecutive nodes (flat index: a run may wrap from one row, or slab, into the next).  The 2x2x2 neighbourhoods of a
// run lie in four spans of MESH_PER + 1 consecutive floats -- at the run, one row up, one slab up, both -- read once each and kept as inside
// bits; a corner outside the grid counts as the node's own side (no active edge), so a span element past the end of the grid only needs to be
// SOMETHING: its index is clamped to the last node.  The divisions that split the flat index are paid once per run.
__global__ __launch_bounds__(MESH_PER_THREADS) void mesh_count_kernel(const float* __restrict__ sigma, uint32_t nx, uint32_t ny, uint32_t nz, uint32_t N,
                                                                      float threshold, MtWorkspace w) {
  __shared__ uint32_t wave_sum[MESH_PER_WAVES];
  const uint32_t tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const uint32_t i0 = blockIdx.x * (uint32_t)MESH_SCAN + MESH_PER * tid;
  uint32_t m[MESH_PER], cnt[MESH_PER];          // cnt: vertices | faces << 16
#pragma unroll
  for (int j = 0; j < MESH_PER; ++j) { m[j] = 0; cnt[j] = 0; }
  if (i0 < N) {
    uint32_t bits[4];
#pragma unroll
    for (int s = 0; s < 4; ++s) {
      const uint64_t at = (uint64_t)i0 + ((s & 1) ? nx : 0u) + ((s & 2) ? (uint64_t)nx * ny : 0ull);
      bits[s] = 0;
#pragma unroll
      for (int k = 0; k <= MESH_PER; ++k) {     // clamped, not skipped: twenty independent loads in flight, no branch and no wait between them
        const uint64_t q = at + k < N ? at + k : (uint64_t)N - 1;
        bits[s] |= (uint32_t)(sigma[q] > threshold) << k;
      }
    }
    uint32_t ix = i0 % nx, r = i0 / nx, iy = r % ny, iz = r / ny;
#pragma unroll
    for (int j = 0; j < MESH_PER; ++j) {
      if (i0 + j < N) {
        const bool vx = ix + 1 < nx, vy = iy + 1 < ny, vz = iz + 1 < nz;
        const uint32_t in0 = (bits[0] >> j) & 1u;
        uint32_t in = in0;                      // bit k: corner k = dx + 2 dy + 4 dz is inside
#pragma unroll
        for (int k = 1; k < 8; ++k) {
          const bool valid = (!(k & 1) || vx) && (!(k & 2) || vy) && (!(k & 4) || vz);
          in |= (valid ? (bits[k >> 1] >> (j + (k & 1))) & 1u : in0) << k;
        }
        m[j] = ((in >> 1) ^ (in0 ? 0x7fu : 0u)) & 0x7fu;
        uint32_t nf = 0;
        if (vx && vy && vz) {
#pragma unroll
          for (int t = 0; t < 6; ++t) {
            const int k1 = 1 << MT_AXES[t][0], k2 = k1 | (1 << MT_AXES[t][1]);
            const uint32_t pc = (in & 1u) + ((in >> k1) & 1u) + ((in >> k2) & 1u) + ((in >> 7) & 1u);
            nf += pc == 2u ? 2u : (pc == 1u || pc == 3u) ? 1u : 0u;
          }
        }
        cnt[j] = (uint32_t)__popc(m[j]) | (nf << 16);
        if (++ix == nx) { ix = 0; if (++iy == ny) { iy = 0; ++iz; } }
      }
    }
  }
  uint32_t own = 0;
#pragma unroll
  for (int j = 0; j < MESH_PER; ++j) own += cnt[j];
  uint32_t total;
  const uint32_t below = block_scan_exclusive<uint32_t, MESH_PER_WAVES, false>(own, wave_sum, lane, wave, total);
  if (i0 < N) {
    uint32_t excl[MESH_PER];
    excl[0] = below;
#pragma unroll
    for (int j = 1; j < MESH_PER; ++j) excl[j] = excl[j - 1] + cnt[j - 1];
    if (i0 + MESH_PER <= N) {                   // i0 is a multiple of 4 and the arrays start on 16 bytes: one store each
      *(uint32_t*)(w.mask + i0) = m[0] | (m[1] << 8) | (m[2] << 16) | (m[3] << 24);
      *(uint2*)(w.vloc + i0) = make_uint2((excl[0] & 0xffffu) | (excl[1] << 16), (excl[2] & 0xffffu) | (excl[3] << 16));
      *(uint2*)(w.floc + i0) = make_uint2((excl[0] >> 16) | (excl[1] & 0xffff0000u), (excl[2] >> 16) | (excl[3] & 0xffff0000u));
    } else {                                    // the grid's last, partial run
#pragma unroll
      for (int j = 0; j < MESH_PER; ++j)
        if (i0 + j < N) {
          w.mask[i0 + j] = (uint8_t)m[j];
          w.vloc[i0 + j] = (uint16_t)(excl[j] & 0xffffu);
          w.floc[i0 + j] = (uint16_t)(excl[j] >> 16);
        }
    }
  }
  if (tid == 0) {
    w.vbase[blockIdx.x] = total & 0xffffu;
    w.fbase[blockIdx.x] = total >> 16;
  }
}
static_assert(MESH_PER == 4, "the packed stores above hold four nodes");

// ---------------------------------------------------------------------------------------------------------------- emit
struct MtGrid {
  const float* sigma; const float* xs; const float* ys; const float* zs;
  uint32_t nx, ny, nz, N;
};

// d sigma / d (x, y, z) at a node: central differences, one-sided at the border, over the actual spacing (every axis has >= 2 nodes here)
__device__ __forceinline__ void mt_gradient(const MtGrid& g, uint32_t ix, uint32_t iy, uint32_t iz, uint32_t idx, float out[3]) {
  const uint32_t sxy = g.nx * g.ny;
  const uint32_t x0 = ix > 0 ? ix - 1 : ix, x1 = ix + 1 < g.nx ? ix + 1 : ix;
  const uint32_t y0 = iy > 0 ? iy - 1 : iy, y1 = iy + 1 < g.ny ? iy + 1 : iy;
  const uint32_t z0 = iz > 0 ? iz - 1 : iz, z1 = iz + 1 < g.nz ? iz + 1 : iz;
  out[0] = (g.sigma[idx + (x1 - ix)] - g.sigma[idx - (ix - x0)]) / (g.xs[x1] - g.xs[x0]);
  out[1] = (g.sigma[idx + (y1 - iy) * g.nx] - g.sigma[idx - (iy - y0) * g.nx]) / (g.ys[y1] - g.ys[y0]);
  out[2] = (g.sigma[idx + (z1 - iz) * sxy] - g.sigma[idx - (iz - z0) * sxy]) / (g.zs[z1] - g.zs[z0]);
}

__device__ __forceinline__ float mt_lerp(float a, float b, float t) { return __fadd_rn(a, __fmul_rn(t, __fsub_rn(b, a))); }

// node i with the non-empty mask m: its vertices and, as a cell's origin, its faces
__device__ __forceinline__ void mt_emit_node(const MtGrid& g, float threshold, const MtWorkspace& w, long long v_cap, long long f_cap,
                                             float* __restrict__ vertices, float* __restrict__ normals, int32_t* __restrict__ faces, uint32_t i,
                                             uint32_t m) {
  const uint32_t ix = i % g.nx, r = i / g.nx, iy = r % g.ny, iz = r / g.ny;
  const uint32_t sxy = g.nx * g.ny;
  const float sa = g.sigma[i];
  const long long voff = (long long)(w.vbase[i >> MESH_SCAN_SHIFT] + w.vloc[i]);

  if (voff < v_cap) {
    const float xa = g.xs[ix], ya = g.ys[iy], za = g.zs[iz];
    float ga[3] = {0.f, 0.f, 0.f};
    if (normals) mt_gradient(g, ix, iy, iz, i, ga);
    long long id = voff;
    for (int d = 0; d < 7; ++d) {
      if (!((m >> d) & 1u)) continue;
      if (id >= v_cap) break;
      const uint32_t dx = (d + 1) & 1, dy = ((d + 1) >> 1) & 1, dz = (d + 1) >> 2;
      const uint32_t q = i + dx + dy * g.nx + dz * sxy;
      const float sb = g.sigma[q];
      float t = __fsub_rn(threshold, sa) / __fsub_rn(sb, sa);
      if (!(t >= 0.f && t <= 1.f)) t = 0.5f;    // (false for a NaN as well)
      float* v = vertices + 3 * id;
      v[0] = mt_lerp(xa, g.xs[ix + dx], t);
      v[1] = mt_lerp(ya, g.ys[iy + dy], t);
      v[2] = mt_lerp(za, g.zs[iz + dz], t);
      if (normals) {
        float gb[3];
        mt_gradient(g, ix + dx, iy + dy, iz + dz, q, gb);
        const float nxv = -mt_lerp(ga[0], gb[0], t), nyv = -mt_lerp(ga[1], gb[1], t), nzv = -mt_lerp(ga[2], gb[2], t);
        const float len = sqrtf(nxv * nxv + nyv * nyv + nzv * nzv);
        const bool ok = len > 0.f && len <= 3.402823466e38f;      // zero, NaN or infinite length: the zero vector
        float* nv = normals + 3 * id;
        nv[0] = ok ? nxv / len : 0.f;
        nv[1] = ok ? nyv / len : 0.f;
        nv[2] = ok ? nzv / len : 0.f;
      }
      ++id;
    }
  }

  if (!(ix + 1 < g.nx && iy + 1 < g.ny && iz + 1 < g.nz)) return;
  long long f = (long long)(w.fbase[i >> MESH_SCAN_SHIFT] + w.floc[i]);
  if (f >= f_cap) return;
  const uint32_t in = ((m << 1) ^ (sa > threshold ? 0xffu : 0u)) & 0xffu;      // bit k: corner k is inside
  for (int t = 0; t < 6; ++t) {
    const int k1 = 1 << MT_AXES[t][0], k2 = k1 | (1 << MT_AXES[t][1]);
    const uint32_t pat = (in & 1u) | (((in >> k1) & 1u) << 1) | (((in >> k2) & 1u) << 2) | (((in >> 7) & 1u) << 3);
    const MtCase& c = MT_TABLE.c[t][pat];
    const int n = c.n;
    if (n == 0) continue;
    long long id[4] = {0, 0, 0, 0};
    int first = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      if (j < n) {
        const uint32_t lo = c.lo[j], d = (uint32_t)c.hi[j] - lo - 1u;       // the lower corner owns the edge; d = its direction index
        const uint32_t q = i + (lo & 1u) + ((lo >> 1) & 1u) * g.nx + (lo >> 2) * sxy;
        id[j] = (long long)(w.vbase[q >> MESH_SCAN_SHIFT] + w.vloc[q]) + __popc((uint32_t)w.mask[q] & ((1u << d) - 1u));
      }
    }
#pragma unroll
    for (int j = 1; j < 4; ++j)
      if (j < n && id[j] < id[first]) first = j;
    long long q0 = id[0], q1 = id[1], q2 = id[2], q3 = id[3];               // rotated: the smallest id first
    if (n == 3) {
      if (first == 1) { q0 = id[1]; q1 = id[2]; q2 = id[0]; }
      else if (first == 2) { q0 = id[2]; q1 = id[0]; q2 = id[1]; }
    } else {
      if (first == 1) { q0 = id[1]; q1 = id[2]; q2 = id[3]; q3 = id[0]; }
      else if (first == 2) { q0 = id[2]; q1 = id[3]; q2 = id[0]; q3 = id[1]; }
      else if (first == 3) { q0 = id[3]; q1 = id[0]; q2 = id[1]; q3 = id[2]; }
    }
    if (f >= f_cap) return;
    int32_t* o = faces + 3 * f;
    o[0] = (int32_t)q0; o[1] = (int32_t)q1; o[2] = (int32_t)q2;
    ++f;
    if (n == 4) {
      if (f >= f_cap) return;
      o = faces + 3 * f;
      o[0] = (int32_t)q0; o[1] = (int32_t)q2; o[2] = (int32_t)q3;
      ++f;
    }
  }
}

// One thread LOADS the masks of MT_EMIT_PER consecutive nodes (16 bytes); most of the grid has none set.  The active nodes of a wave's 1,024 are
// queued in LDS -- slots from an LDS counter: the order in the queue is arbitrary and does not matter, every output row is addressed by its id --
// and the wave's lanes then take one queued node each, so the long, dependent walk of an active node (offsets, sigma, axes, gradients) runs 64
// wide however the surface lies to the rows.
constexpr int MT_EMIT_PER = 16;
constexpr int MT_EMIT_WAVES = MT_EMIT_THREADS / 64;
constexpr int MT_EMIT_WAVE_NODES = 64 * MT_EMIT_PER;

__global__ __launch_bounds__(MT_EMIT_THREADS) void mesh_emit_kernel(MtGrid g, float threshold, MtWorkspace w, long long v_cap, long long f_cap,
                                                                    float* __restrict__ vertices, float* __restrict__ normals,
                                                                    int32_t* __restrict__ faces) {
  __shared__ uint32_t queue[MT_EMIT_WAVES][MT_EMIT_WAVE_NODES];      // (node - the wave's first node) << 8 | mask
  __shared__ uint32_t queued[MT_EMIT_WAVES];
  const uint32_t tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const uint64_t run = (uint64_t)blockIdx.x * MT_EMIT_THREADS + tid;
  const uint64_t wave_first = ((uint64_t)blockIdx.x * MT_EMIT_THREADS + 64 * wave) * MT_EMIT_PER;
  unsigned long long w0 = 0ull, w1 = 0ull;
  if (run * MT_EMIT_PER < g.N) {
    const uint32_t i0 = (uint32_t)(run * MT_EMIT_PER);
    if (g.N - i0 >= (uint32_t)MT_EMIT_PER) {    // (the mask array starts on 16 bytes)
      const uint4 q = *(const uint4*)(w.mask + i0);
      w0 = q.x | ((unsigned long long)q.y << 32);
      w1 = q.z | ((unsigned long long)q.w << 32);
    } else {                                    // the grid's last, partial run
      for (uint32_t j = 0; i0 + j < g.N; ++j) {
        const unsigned long long b = (unsigned long long)w.mask[i0 + j] << (8 * (j & 7));
        if (j < 8) w0 |= b; else w1 |= b;
      }
    }
  }
  if (lane == 0) queued[wave] = 0;
  __syncthreads();
  if (w0 | w1) {
    uint32_t c = 0;
    for (int j = 0; j < MT_EMIT_PER; ++j) c += ((j < 8 ? w0 >> (8 * j) : w1 >> (8 * (j - 8))) & 0xffull) != 0ull;
    uint32_t slot = atomicAdd(&queued[wave], c);                     // c <= 16 a lane: slot + c <= MT_EMIT_WAVE_NODES
    for (int j = 0; j < MT_EMIT_PER; ++j) {
      const uint32_t m = (uint32_t)((j < 8 ? w0 >> (8 * j) : w1 >> (8 * (j - 8))) & 0xffull);
      if (m) queue[wave][slot++] = ((MT_EMIT_PER * lane + j) << 8) | m;
    }
  }
  __syncthreads();
  const uint32_t n = queued[wave];
  for (uint32_t k = lane; k < n; k += 64) {
    const uint32_t e = queue[wave][k];
    mt_emit_node(g, threshold, w, v_cap, f_cap, vertices, normals, faces, (uint32_t)(wave_first + (e >> 8)), e & 0xffu);
  }
}

// ---------------------------------------------------------------------------------------------------------------- host
// negative: refused.  0 with *empty set: nothing to do (an empty axis, or one shorter than 2: no cell)
static int mt_shape(const char* who, int32_t nx, int32_t ny, int32_t nz, bool* empty) {
  *empty = false;
  if (nx < 0 || ny < 0 || nz < 0) return launch_fail(CRNERF_ERR_SHAPE, who, "negative axis length");
  if (nx == 0 || ny == 0 || nz == 0) { *empty = true; return 0; }
  // (nx * ny < 2^62, and the quotient test keeps the triple product out of 64-bit overflow)
  if ((int64_t)nx * ny > MESH_MAX / nz) return launch_fail(CRNERF_ERR_SHAPE, who, "more than 2^31 - 1 nodes in one call");
  if (nx < 2 || ny < 2 || nz < 2) *empty = true;
  return 0;
}

}  // namespace crnerf

using namespace crnerf;

#define MT_REQUIRE(p, name) \
  if (!(p)) return set_error(CRNERF_ERR_NULL, name " is NULL")

extern "C" size_t crnerf_mesh_workspace_bytes(int32_t nx, int32_t ny, int32_t nz) {
  if (nx <= 0 || ny <= 0 || nz <= 0 || (int64_t)nx * ny > MESH_MAX / nz) return 0;
  const uint32_t N = (uint32_t)((int64_t)nx * ny * nz);
  return (size_t)16 * scan_blocks(N) + (size_t)5 * N + MT_WORKSPACE_PAD;
}

extern "C" int crnerf_mesh_count_f32(const float* sigma, int32_t nx, int32_t ny, int32_t nz, float threshold, void* workspace, int64_t* counts,
                                     void* stream) {
  bool empty;
  if (int rc = mt_shape("mesh_count", nx, ny, nz, &empty)) return rc;
  if (empty) {                                  // no cell: V = F = 0, nothing is launched
    if (counts && hipMemsetAsync(counts, 0, 2 * sizeof(int64_t), (hipStream_t)stream) != hipSuccess)
      return set_error(CRNERF_ERR_HIP, "mesh_count: hipMemsetAsync(counts) failed");
    return 0;
  }
  MT_REQUIRE(sigma, "sigma"); MT_REQUIRE(workspace, "workspace"); MT_REQUIRE(counts, "counts");
  MESH_ALIGNED(workspace, "mesh_count");
  hipStream_t st = (hipStream_t)stream;
  const uint32_t N = (uint32_t)((int64_t)nx * ny * nz), nb = scan_blocks(N);
  const MtWorkspace w = mt_carve(workspace, N);
  if (int rc = mesh_launch(mesh_count_kernel, "mesh_count_kernel", nb, MESH_PER_THREADS, st, sigma, (uint32_t)nx, (uint32_t)ny, (uint32_t)nz, N, threshold, w))
    return rc;
  long long* const out = (long long*)counts;
  return mesh_block_scan(st, ScanList<1>{w.vbase, nb, {out}}, ScanList<1>{w.fbase, nb, {out + 1}});
}

extern "C" int crnerf_mesh_emit_f32(const float* sigma, const float* xs, const float* ys, const float* zs, int32_t nx, int32_t ny, int32_t nz,
                                    float threshold, const void* workspace, int64_t v_cap, int64_t f_cap, float* vertices, float* normals,
                                    int32_t* faces, void* stream) {
  bool empty;
  if (int rc = mt_shape("mesh_emit", nx, ny, nz, &empty)) return rc;
  if (int rc = mesh_caps("mesh_emit", v_cap, f_cap)) return rc;
  if (empty || (v_cap == 0 && f_cap == 0)) return 0;
  MT_REQUIRE(sigma, "sigma"); MT_REQUIRE(xs, "xs"); MT_REQUIRE(ys, "ys"); MT_REQUIRE(zs, "zs"); MT_REQUIRE(workspace, "workspace");
  if (v_cap > 0) MT_REQUIRE(vertices, "vertices");
  if (f_cap > 0) MT_REQUIRE(faces, "faces");
  MESH_ALIGNED(workspace, "mesh_emit");
  const uint32_t N = (uint32_t)((int64_t)nx * ny * nz);
  const MtWorkspace w = mt_carve(const_cast<void*>(workspace), N);
  const MtGrid g{sigma, xs, ys, zs, (uint32_t)nx, (uint32_t)ny, (uint32_t)nz, N};
  return mesh_launch(mesh_emit_kernel, "mesh_emit_kernel", launch_blocks(N, MT_EMIT_THREADS * MT_EMIT_PER), MT_EMIT_THREADS, (hipStream_t)stream, g, threshold,
                     w, (long long)v_cap, (long long)f_cap, vertices, normals, faces);
}

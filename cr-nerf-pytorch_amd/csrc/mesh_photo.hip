// Photo colours for meshes (csrc/crnerf_mesh_photo.h carries every rule): a z-buffer of the mesh in N posed pinhole views, and the
// fused project / test / sample / average pass per vertex over N posed photos.  Screen coordinates on a 1/16-pixel integer lattice, coverage by
// exact integer edge functions, depths through an integer atomic minimum, colours from 64-bit integer sums -- the same bytes on every run,
// whatever the order of the faces.
//
// Z-buffer: (fill) depth = +inf; zbuffer_kernel, one thread per (face, view) pair.  The view is blockIdx.y (a grid-stride loop above 65,535 views),
//   so a view's camera, size and offset are the same in every lane of a workgroup and travel through scalar loads.  Marching-tetrahedra faces are
//   mostly below a pixel: a bounding box of at most ZB_WAVE pixels is walked by the thread itself; a larger one is handed to the wave -- the
//   owner's corners go round by shuffles and the 64 lanes take the box's pixels 64 a trip.  Every lane stays to the end of the view loop (the
//   shuffles need them all).
// Colours: photo_colors_kernel, one thread per vertex, looping over the views; the table entries of a view are wave-uniform (scalar loads), the
//   three sums and the count stay in registers, no atomics; the 2 x 2 x 3 bytes of a sample and the one depth are the only divergent loads.
//
// Bounds.  A view's W, H and offset are used only after ph_view has held them to the buffer (W, H in [2, 16384], 0 <= off, off + W H <= total);
// a pixel index is formed only from i in [0, W - 1] and j in [0, H - 1].  A face's ids are tested by load_face before a vertex is read.
// Coherence.  depth[] is touched with atomics only inside zbuffer_kernel; the colour launch reads it plainly (mesh_parts.hip).
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include "crnerf_mesh_photo.h"
#include "mesh_common.h"

namespace crnerf {

constexpr uint32_t ZB_WAVE = 16;                // pixels: a larger bounding box is walked by the wave together
constexpr int32_t PH_MAX_SIDE = 16384;
constexpr double PH_MAX_UV = 1048576.0;         // 2^20 pixels: |X|, |Y| <= 2^24 fit an int32, their differences too
constexpr int64_t PH_MAX_PIXELS = 1ll << 40;
constexpr uint32_t PH_MAX_GRID_Y = 65535;
constexpr uint32_t PH_INF_BITS = 0x7F800000u;

// W, H and off of view n and true; false for a view that is skipped.  Nothing of a skipped view is used.
__device__ __forceinline__ bool ph_view(const int32_t* __restrict__ dims, const long long* __restrict__ offsets, uint32_t n, long long total,
                                        int32_t& W, int32_t& H, long long& off) {
  W = dims[2 * (size_t)n];
  H = dims[2 * (size_t)n + 1];
  off = offsets[n];
  if (W < 2 || H < 2 || W > PH_MAX_SIDE || H > PH_MAX_SIDE) return false;
  if (off < 0) return false;
  return off <= total - (long long)W * (long long)H;      // (W H <= 2^28 and total >= 0: no overflow)
}

// The projection of crnerf_mesh_photo.h; cam: the 16 doubles of the view.  d[] is left for the facing test.  True iff the point is in front.
__device__ __forceinline__ bool ph_project(const double* __restrict__ cam, const float x[3], double z_near, double d[3], double& u, double& v,
                                           double& z) {
  const double* R = cam + 4;
  const double* t = cam + 13;
#pragma unroll
  for (int a = 0; a < 3; ++a) d[a] = (double)x[a] - t[a];
  double c[3];
#pragma unroll
  for (int k = 0; k < 3; ++k) c[k] = (d[0] * R[k] + d[1] * R[3 + k]) + d[2] * R[6 + k];
  z = -c[2];
  u = cam[2] + cam[0] * (c[0] / z);
  v = cam[3] - cam[1] * (c[1] / z);
  return z >= z_near;
}

// ---------------------------------------------------------------------------------------------------------------- z-buffer
struct ZbTri {
  int32_t X[3], Y[3];       // on the 1/16-pixel lattice, corners 1 and 2 exchanged where the face was clockwise
  double z[3];
  long long A;              // > 0
  int32_t i0, j0, w;        // the box: first column, first row, columns
  uint32_t count;           // pixels of the box; 0: nothing to draw
};

__device__ __forceinline__ void zb_pixel(const ZbTri& t, int32_t i, int32_t j, uint32_t* __restrict__ row) {
  const int32_t px = 16 * i, py = 16 * j;
  const long long e0 = (long long)(t.X[2] - t.X[1]) * (long long)(py - t.Y[1]) - (long long)(t.Y[2] - t.Y[1]) * (long long)(px - t.X[1]);
  const long long e1 = (long long)(t.X[0] - t.X[2]) * (long long)(py - t.Y[2]) - (long long)(t.Y[0] - t.Y[2]) * (long long)(px - t.X[2]);
  const long long e2 = (long long)(t.X[1] - t.X[0]) * (long long)(py - t.Y[0]) - (long long)(t.Y[1] - t.Y[0]) * (long long)(px - t.X[0]);
  if (e0 < 0 || e1 < 0 || e2 < 0) return;
  const double a = (double)t.A;
  const double w0 = (double)e0 / a, w1 = (double)e1 / a, w2 = (double)e2 / a;
  const double iz = (w0 / t.z[0] + w1 / t.z[1]) + w2 / t.z[2];
  const float D = (float)(1.0 / iz);
  atomicMin(row + i, __float_as_uint(D));      // i in [0, W - 1]: the box is clipped to the view
}

__global__ __launch_bounds__(MESH_THREADS) void zbuffer_kernel(const float* __restrict__ vertices, const int32_t* __restrict__ faces, uint32_t V,
                                                             uint32_t F, const double* __restrict__ cams, const int32_t* __restrict__ dims,
                                                             const long long* __restrict__ offsets, uint32_t N, long long total, double z_near,
                                                             uint32_t* __restrict__ depth) {
  const uint32_t f = blockIdx.x * (uint32_t)MESH_THREADS + threadIdx.x, lane = threadIdx.x & 63;
  int32_t id[3];
  const bool valid = load_face(faces, f, F, V, id);
  float x[3][3] = {};
  if (valid) {
#pragma unroll
    for (int k = 0; k < 3; ++k)
#pragma unroll
      for (int a = 0; a < 3; ++a) x[k][a] = vertices[3 * (size_t)id[k] + a];
  }
  for (uint32_t n = blockIdx.y; n < N; n += gridDim.y) {      // (the same trips in every lane of the workgroup)
    int32_t W, H;
    long long off;
    if (!ph_view(dims, offsets, n, total, W, H, off)) continue;
    const double* cam = cams + 16 * (size_t)n;
    ZbTri t = {};
    if (valid) {
      double u[3], v[3], d[3];
      bool draw = true;
#pragma unroll
      for (int k = 0; k < 3; ++k) {
        const bool front = ph_project(cam, x[k], z_near, d, u[k], v[k], t.z[k]);
        draw = draw && front && fabs(u[k]) < PH_MAX_UV && fabs(v[k]) < PH_MAX_UV;
      }
      if (draw) {
#pragma unroll
        for (int k = 0; k < 3; ++k) {
          t.X[k] = (int32_t)rint(u[k] * 16.0);
          t.Y[k] = (int32_t)rint(v[k] * 16.0);
        }
        t.A = (long long)(t.X[1] - t.X[0]) * (long long)(t.Y[2] - t.Y[0]) - (long long)(t.Y[1] - t.Y[0]) * (long long)(t.X[2] - t.X[0]);
        if (t.A < 0) {
          int32_t s = t.X[1]; t.X[1] = t.X[2]; t.X[2] = s;
          s = t.Y[1]; t.Y[1] = t.Y[2]; t.Y[2] = s;
          const double zs = t.z[1]; t.z[1] = t.z[2]; t.z[2] = zs;
          t.A = -t.A;
        }
        if (t.A != 0) {
          const int32_t minx = min(t.X[0], min(t.X[1], t.X[2])), maxx = max(t.X[0], max(t.X[1], t.X[2]));
          const int32_t miny = min(t.Y[0], min(t.Y[1], t.Y[2])), maxy = max(t.Y[0], max(t.Y[1], t.Y[2]));
          const int32_t i0 = max(0, (minx + 15) >> 4), i1 = min(W - 1, maxx >> 4);      // (an arithmetic shift: floor for a negative bound too)
          const int32_t j0 = max(0, (miny + 15) >> 4), j1 = min(H - 1, maxy >> 4);
          if (i0 <= i1 && j0 <= j1) {
            t.i0 = i0; t.j0 = j0; t.w = i1 - i0 + 1;
            t.count = (uint32_t)t.w * (uint32_t)(j1 - j0 + 1);      // at most 2^28
          }
        }
      }
    }
    uint32_t* view = depth + off;
    if (t.count != 0 && t.count <= ZB_WAVE) {
      const int32_t h = (int32_t)(t.count / (uint32_t)t.w);
      for (int32_t j = t.j0; j < t.j0 + h; ++j)
        for (int32_t i = t.i0; i < t.i0 + t.w; ++i) zb_pixel(t, i, j, view + (size_t)j * (size_t)W);
    }
    // the large boxes of this wave, one after another, 64 pixels a trip; every lane takes part
    unsigned long long todo = __ballot(t.count > ZB_WAVE);
    while (todo) {
      const int owner = __ffsll((long long)todo) - 1;
      todo &= todo - 1;
      ZbTri o;
#pragma unroll
      for (int k = 0; k < 3; ++k) {
        o.X[k] = __shfl(t.X[k], owner, 64);
        o.Y[k] = __shfl(t.Y[k], owner, 64);
        o.z[k] = __shfl(t.z[k], owner, 64);
      }
      o.A = __shfl(t.A, owner, 64);
      o.i0 = __shfl(t.i0, owner, 64);
      o.j0 = __shfl(t.j0, owner, 64);
      o.w = __shfl(t.w, owner, 64);
      o.count = __shfl(t.count, owner, 64);
      for (uint32_t p = lane; p < o.count; p += 64) {
        const int32_t j = o.j0 + (int32_t)(p / (uint32_t)o.w), i = o.i0 + (int32_t)(p % (uint32_t)o.w);
        zb_pixel(o, i, j, view + (size_t)j * (size_t)W);
      }
    }
  }
}

// ---------------------------------------------------------------------------------------------------------------- colours
__global__ __launch_bounds__(MESH_THREADS) void photo_colors_kernel(const float* __restrict__ vertices, const float* __restrict__ normals, uint32_t V,
                                                                  const uint8_t* __restrict__ photos, const float* __restrict__ depth,
                                                                  const double* __restrict__ cams, const int32_t* __restrict__ dims,
                                                                  const long long* __restrict__ offsets, uint32_t N, long long total, double z_near,
                                                                  double s, float* __restrict__ out_colors, int32_t* __restrict__ out_views) {
  const uint32_t i = blockIdx.x * (uint32_t)MESH_THREADS + threadIdx.x;
  if (i >= V) return;
  float x[3];
  double nrm[3] = {0.0, 0.0, 0.0};
#pragma unroll
  for (int a = 0; a < 3; ++a) x[a] = vertices[3 * (size_t)i + a];
  bool facing = false;
  if (normals) {
#pragma unroll
    for (int a = 0; a < 3; ++a) nrm[a] = (double)normals[3 * (size_t)i + a];
    facing = !(nrm[0] == 0.0 && nrm[1] == 0.0 && nrm[2] == 0.0);
  }
  long long sum[3] = {0, 0, 0};
  int32_t cnt = 0;
  for (uint32_t n = 0; n < N; ++n) {
    int32_t W, H;
    long long off;
    if (!ph_view(dims, offsets, n, total, W, H, off)) continue;
    double d[3], u, v, z;
    if (!ph_project(cams + 16 * (size_t)n, x, z_near, d, u, v, z)) continue;
    if (facing) {
      const double g = -((nrm[0] * d[0] + nrm[1] * d[1]) + nrm[2] * d[2]);
      if (!(g > 0.0)) continue;
    }
    if (!(u >= 0.0 && u <= (double)(W - 1) && v >= 0.0 && v <= (double)(H - 1))) continue;
    if (depth) {
      const int32_t pi = (int32_t)rint(u), pj = (int32_t)rint(v);      // in [0, W - 1] and [0, H - 1]
      const double D = (double)depth[off + (long long)pj * W + pi];
      if (!(z <= D * s)) continue;
    }
    const int32_t x0 = min((int32_t)floor(u), W - 2), y0 = min((int32_t)floor(v), H - 2);
    const double a = u - (double)x0, b = v - (double)y0;
    const uint8_t* top = photos + 3 * (off + (long long)y0 * W + x0);      // (x0, y0) and (x0 + 1, y0): six bytes; the row below: 3 W on
    const uint8_t* bot = top + 3 * (long long)W;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const double p00 = (double)top[c], p10 = (double)top[3 + c], p01 = (double)bot[c], p11 = (double)bot[3 + c];
      const double tv = p00 + a * (p10 - p00);
      const double bv = p01 + a * (p11 - p01);
      const double val = tv + b * (bv - tv);
      sum[c] += (long long)rint(val * 65536.0);
    }
    ++cnt;
  }
  out_views[i] = cnt;
#pragma unroll
  for (int c = 0; c < 3; ++c) out_colors[3 * (size_t)i + c] = cnt ? (float)((double)sum[c] / ((double)cnt * 16711680.0)) : 0.0f;
}

static int ph_sizes(const char* who, int64_t V, int64_t F, int64_t N, int64_t total_pixels, double z_near) {
  if (int rc = mesh_sizes(who, V, F)) return rc;
  if (N < 0) return launch_fail(CRNERF_ERR_SHAPE, who, "negative size");
  if (N > MESH_MAX) return launch_fail(CRNERF_ERR_SHAPE, who, "more than 2^31 - 1 views in one call");
  if (total_pixels < 0 || total_pixels > PH_MAX_PIXELS) return launch_fail(CRNERF_ERR_SHAPE, who, "total_pixels outside [0, 2^40]");
  if (!std::isfinite(z_near) || !(z_near > 0.0)) return launch_fail(CRNERF_ERR_SHAPE, who, "a z_near that is not finite or <= 0");
  return 0;
}

}  // namespace crnerf

// ---------------------------------------------------------------------------------------------------------------- host
using namespace crnerf;

extern "C" int crnerf_mesh_zbuffer_f32(const float* vertices, const int32_t* faces, int64_t V, int64_t F, const double* cams, const int32_t* dims,
                                       const int64_t* offsets, int64_t N, int64_t total_pixels, double z_near, float* depth, void* stream) {
  static const char* who = "mesh_zbuffer";
  if (int rc = ph_sizes(who, V, F, N, total_pixels, z_near)) return rc;
  if (total_pixels == 0) return 0;
  MESH_REQUIRE(depth, who, "depth");
  const bool draw = N > 0 && F > 0;
  if (draw) {
    MESH_REQUIRE(faces, who, "faces"); MESH_REQUIRE(cams, who, "cams"); MESH_REQUIRE(dims, who, "dims"); MESH_REQUIRE(offsets, who, "offsets");
    if (V > 0) MESH_REQUIRE(vertices, who, "vertices");
  }
  hipStream_t st = (hipStream_t)stream;
  if (hipMemsetD32Async((hipDeviceptr_t)depth, (int)PH_INF_BITS, (size_t)total_pixels, st) != hipSuccess)
    return launch_fail(CRNERF_ERR_HIP, who, "hipMemsetD32Async failed");
  if (!draw) return 0;
  const dim3 grid(launch_blocks((uint64_t)F, MESH_THREADS), (uint32_t)(N < (int64_t)PH_MAX_GRID_Y ? N : (int64_t)PH_MAX_GRID_Y));
  hipLaunchKernelGGL(zbuffer_kernel, grid, dim3(MESH_THREADS), 0, st, vertices, faces, (uint32_t)V, (uint32_t)F, cams, dims, (const long long*)offsets,
                     (uint32_t)N, (long long)total_pixels, z_near, (uint32_t*)depth);
  return check_launch("zbuffer_kernel");
}

extern "C" int crnerf_mesh_photo_colors_u8(const float* vertices, const float* normals, int64_t V, const uint8_t* photos, const float* depth,
                                           const double* cams, const int32_t* dims, const int64_t* offsets, int64_t N, int64_t total_pixels,
                                           double z_near, double depth_tol, float* out_colors, int32_t* out_views, void* stream) {
  static const char* who = "mesh_photo_colors";
  if (int rc = ph_sizes(who, V, 0, N, total_pixels, z_near)) return rc;
  if (!std::isfinite(depth_tol) || depth_tol < 0.0) return launch_fail(CRNERF_ERR_SHAPE, who, "a depth_tol that is not finite or < 0");
  if (V == 0) return 0;
  MESH_REQUIRE(vertices, who, "vertices"); MESH_REQUIRE(out_colors, who, "out_colors"); MESH_REQUIRE(out_views, who, "out_views");
  if (N > 0) {
    MESH_REQUIRE(cams, who, "cams"); MESH_REQUIRE(dims, who, "dims"); MESH_REQUIRE(offsets, who, "offsets");
    if (total_pixels > 0) MESH_REQUIRE(photos, who, "photos");
  }
  return mesh_launch(photo_colors_kernel, "photo_colors_kernel", launch_blocks((uint64_t)V, MESH_THREADS), MESH_THREADS, (hipStream_t)stream, vertices,
                     normals, (uint32_t)V, photos, depth, cams, dims, (const long long*)offsets, (uint32_t)N, (long long)total_pixels, z_near,
                     1.0 + depth_tol, out_colors, out_views);
}

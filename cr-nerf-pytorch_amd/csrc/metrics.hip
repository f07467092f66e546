// Evaluation metrics of a rendered image: sum of squared differences and SSIM of a region of
// interest, both images read once, in place, through element strides.
//
// Reference: metrics.py:4-20 (mse / psnr / ssim = kornia.metrics.ssim(img1, img2, 3)), scored on the right half of a
//            Phototourism test image by eval_metric.py:87-93 after the PNG round trip of eval.py:296-297.
// SSIM, restated (include/crnerf.h carries the definition): 3x3 Gaussian window (sigma 1.5), reflect border relative
// to the ROI, C1 = 0.01^2, C2 = 0.03^2, eps = 1e-12.  The second moments are evaluated CENTRED -- sum w (a - mu)^2 --
// which is the same number as E[a^2] - mu^2 without its cancellation.
// No roofline is claimed: an 800x800 frame is 15 MB of reads, the launch dominates (as with cgnet.hip).
#include <hip/hip_runtime.h>
#include "kernels.h"

namespace crnerf {

constexpr int MET_THREADS = 256;
constexpr int MET_ROWS = METRICS_TILE_H / (MET_THREADS / METRICS_TILE_W);    // pixels (rows) per thread
constexpr int MET_LW = METRICS_TILE_W + 2, MET_LH = METRICS_TILE_H + 2;      // tile + one-pixel halo
static_assert(MET_THREADS % METRICS_TILE_W == 0 && METRICS_TILE_H % (MET_THREADS / METRICS_TILE_W) == 0, "tile / thread map");

// g = exp(-x^2 / (2 * 1.5^2)), x = -1, 0, 1, normalised: [0.30780133, 0.38439734, 0.30780133]; the 2-D window is g g^T
constexpr float MET_WC = 0.09474165821017468f, MET_WE = 0.11831801270312059f, MET_WM = 0.1477613163468188f;   // corner, edge, middle
constexpr float MET_C1 = 0.0001f, MET_C2 = 0.0009f, MET_EPS = 1e-12f;

// torch's 'reflect' padding by one pixel: -1 -> 1, n -> n - 2 (n >= 2)
__device__ __forceinline__ int reflect1(int i, int n) { return i < 0 ? -i : (i >= n ? 2 * n - 2 - i : i); }

__device__ __forceinline__ float win9(const float (&v)[9]) {
  float s = MET_WC * v[0];
  s = fmaf(MET_WE, v[1], s); s = fmaf(MET_WC, v[2], s);
  s = fmaf(MET_WE, v[3], s); s = fmaf(MET_WM, v[4], s); s = fmaf(MET_WE, v[5], s);
  s = fmaf(MET_WC, v[6], s); s = fmaf(MET_WE, v[7], s); s = fmaf(MET_WC, v[8], s);
  return s;
}

// one workgroup = one METRICS_TILE_H x METRICS_TILE_W tile of one channel; partial[block] = {sse, sum of the SSIM map} of the tile
__global__ __launch_bounds__(MET_THREADS) void image_metrics_kernel(MetricsArgs a, int tiles_x, int tiles_y, double* __restrict__ partial,
                                                                    float* __restrict__ map) {
  __shared__ float sa[MET_LH][MET_LW], sb[MET_LH][MET_LW];
  __shared__ double red[MET_THREADS / 64][2];
  const long blk = blockIdx.x;
  const int tile_x = (int)(blk % tiles_x), tile_y = (int)((blk / tiles_x) % tiles_y), c = (int)(blk / ((long)tiles_x * tiles_y));
  const int X0 = tile_x * METRICS_TILE_W, Y0 = tile_y * METRICS_TILE_H;
  const float* __restrict__ pp = a.pred + (long)c * a.p_sc;
  const float* __restrict__ gp = a.gt + (long)c * a.g_sc;
  for (int i = threadIdx.x; i < MET_LH * MET_LW; i += MET_THREADS) {
    const int ly = i / MET_LW, lx = i - ly * MET_LW;
    int ry = Y0 + ly - 1, rx = X0 + lx - 1;        // ROI coordinates of this tile element
    float p = 0.0f, g = 0.0f;
    if (ry >= -1 && ry <= a.h && rx >= -1 && rx <= a.w) {     // inside the ROI or its one-pixel border; the rest of an edge tile is never used
      ry = reflect1(ry, a.h); rx = reflect1(rx, a.w);
      p = pp[(long)(a.y0 + ry) * a.p_sy + (long)(a.x0 + rx) * a.p_sx];
      g = gp[(long)(a.y0 + ry) * a.g_sy + (long)(a.x0 + rx) * a.g_sx];
      if (a.quantize_pred) p = truncf(fminf(fmaxf(p, 0.0f), 1.0f) * 255.0f) / 255.0f;   // eval.py:296-297 + ToTensor: a true division
    }
    sa[ly][lx] = p; sb[ly][lx] = g;
  }
  __syncthreads();
  const int tx = threadIdx.x % METRICS_TILE_W, ty = (threadIdx.x / METRICS_TILE_W) * MET_ROWS;
  double sse = 0.0, ssum = 0.0;
#pragma unroll
  for (int r = 0; r < MET_ROWS; ++r) {
    const int y = Y0 + ty + r, x = X0 + tx;
    if (y >= a.h || x >= a.w) continue;
    float va[9], vb[9];
#pragma unroll
    for (int j = 0; j < 3; ++j)
#pragma unroll
      for (int i = 0; i < 3; ++i) {
        va[j * 3 + i] = sa[ty + r + j][tx + i];
        vb[j * 3 + i] = sb[ty + r + j][tx + i];
      }
    const double d = (double)va[4] - (double)vb[4];
    sse += d * d;
    const float mu1 = win9(va), mu2 = win9(vb);
    float q11[9], q22[9], q12[9];
#pragma unroll
    for (int k = 0; k < 9; ++k) {
      const float da = va[k] - mu1, db = vb[k] - mu2;
      q11[k] = da * da; q22[k] = db * db; q12[k] = da * db;
    }
    const float s11 = win9(q11), s22 = win9(q22), s12 = win9(q12);
    const float num = (2.0f * (mu1 * mu2) + MET_C1) * (2.0f * s12 + MET_C2);
    const float den = ((mu1 * mu1 + mu2 * mu2) + MET_C1) * ((s11 + s22) + MET_C2);
    const float v = num / (den + MET_EPS);
    ssum += (double)v;
    if (map) map[((long)c * a.h + y) * a.w + x] = v;
  }
  // fixed order: lanes of a wave (xor tree), then the waves in index order
#pragma unroll
  for (int s = 32; s >= 1; s >>= 1) { sse += __shfl_xor(sse, s); ssum += __shfl_xor(ssum, s); }
  if ((threadIdx.x & 63) == 0) { red[threadIdx.x >> 6][0] = sse; red[threadIdx.x >> 6][1] = ssum; }
  __syncthreads();
  if (threadIdx.x < 2) {
    double t = red[0][threadIdx.x];
#pragma unroll
    for (int w = 1; w < MET_THREADS / 64; ++w) t += red[w][threadIdx.x];
    partial[blk * 2 + threadIdx.x] = t;
  }
}

// one workgroup: thread t adds partial[t], partial[t + 256], ... in that order, then a fixed LDS tree -> out2 = {sse, ssim_sum}
__global__ __launch_bounds__(MET_THREADS) void image_metrics_final_kernel(const double* __restrict__ partial, long nblk, double* __restrict__ out2) {
  __shared__ double red[MET_THREADS][2];
  double s0 = 0.0, s1 = 0.0;
  for (long b = threadIdx.x; b < nblk; b += MET_THREADS) { s0 += partial[b * 2]; s1 += partial[b * 2 + 1]; }
  red[threadIdx.x][0] = s0; red[threadIdx.x][1] = s1;
  __syncthreads();
  for (int s = MET_THREADS / 2; s >= 1; s >>= 1) {
    if ((int)threadIdx.x < s) { red[threadIdx.x][0] += red[threadIdx.x + s][0]; red[threadIdx.x][1] += red[threadIdx.x + s][1]; }
    __syncthreads();
  }
  if (threadIdx.x < 2) out2[threadIdx.x] = red[0][threadIdx.x];
}

long image_metrics_blocks(int channels, int w, int h) {
  const long tx = (w + METRICS_TILE_W - 1) / METRICS_TILE_W, ty = (h + METRICS_TILE_H - 1) / METRICS_TILE_H;
  return tx * ty * channels;
}

size_t image_metrics_workspace_bytes(int channels, int w, int h) { return (size_t)image_metrics_blocks(channels, w, h) * 2 * sizeof(double); }

int launch_image_metrics(const MetricsArgs& a, double* out2, float* ssim_map, void* workspace, hipStream_t stream) {
  const int tiles_x = (a.w + METRICS_TILE_W - 1) / METRICS_TILE_W, tiles_y = (a.h + METRICS_TILE_H - 1) / METRICS_TILE_H;
  const long nblk = image_metrics_blocks(a.channels, a.w, a.h);
  hipLaunchKernelGGL(image_metrics_kernel, dim3((unsigned)nblk), dim3(MET_THREADS), 0, stream, a, tiles_x, tiles_y, (double*)workspace, ssim_map);
  hipLaunchKernelGGL(image_metrics_final_kernel, dim3(1), dim3(MET_THREADS), 0, stream, (const double*)workspace, nblk, out2);
  return check_launch("image_metrics");
}

}  // namespace crnerf

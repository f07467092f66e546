// LPIPS (AlexNet backbone, version 0.1) of a region of interest of an image pair -- the third column of the reference's result.txt
// (eval_metric.py:90-93, lpips.LPIPS(net='alex')), restated from its definition (include/crnerf.h carries it; the lpips package and
// torchvision are not needed and no weights are shipped: the caller hands in the 17 tensors).
//
// Layout: activations are pixel-major, [image][y][x][c], BOTH images stacked along the GEMM's m.  A convolution is an NT GEMM on
// v_mfma_f32_32x32x2_f32 (the pattern of encoder.hip): A = the patch matrix X[m][k], m = (image, oy, ox), k = (c, ky, kx) in the
// weight tensor's own order, zeros outside the map; B = the module's own [cout][cin k k] tensor, untouched (conv1's K = 363 is the
// exception: its rows are not 16-byte aligned, a zero-padded [64][368] copy is made in the workspace by the launch that builds X1).
// One workgroup = one 32 x 32 tile of the output, its four waves split K into fixed ranges and their partial tiles are added in
// wave order: the order of k inside a dot product depends on K alone, never on where in m a pixel sits -- so lpips(a, b) and
// lpips(b, a) see the same feature bits, and lpips(a, a) is exactly 0.
// The input stage (ROI, element strides, optional uint8 round trip of the prediction, optional * 2 - 1, scaling layer) is part of
// the gather that builds X1: both images are read in place, nothing outside the ROI is touched, the zero padding sits at its border.
// The head sums in double per workgroup and a one-workgroup kernel adds the partials in a fixed order (no atomics), as metrics.hip.
// No roofline is claimed: a 340 x 257 half image is ~2.3 GFLOP per image in 14 launches, the call is launch-bound (as cgnet.hip).
#include <hip/hip_runtime.h>
#include "kernels.h"

namespace crnerf {

typedef float lp_f32x16 __attribute__((ext_vector_type(16)));
typedef float lp_f32x4 __attribute__((ext_vector_type(4)));

constexpr int LP_LAYERS = 5;
constexpr int LP_CIN[LP_LAYERS] = {3, 64, 192, 384, 256}, LP_COUT[LP_LAYERS] = {64, 192, 384, 256, 256};
constexpr int LP_KS[LP_LAYERS] = {11, 5, 3, 3, 3}, LP_PAD[LP_LAYERS] = {2, 2, 1, 1, 1};
constexpr int LP_C1 = 64, LP_K1 = 3 * 11 * 11, LP_K1P = 368;         // conv1's K and its multiple of 8
constexpr int LP_HEAD_PX = 16;                            // pixels one workgroup of the head sums (four per wave)
constexpr float LP_EPS = 1e-10f;
static_assert(LP_C1 == LP_COUT[0] && LP_K1P % 8 == 0 && LP_K1P >= LP_K1 && LP_K1P - LP_K1 < 8, "conv1 K padding");

struct LpipsGeom {
  int fh[LP_LAYERS], fw[LP_LAYERS];     // feature maps F1..F5
  int ph[2], pw[2];                     // the two pooled maps
  long px[LP_LAYERS];                   // fh * fw
  int kp[LP_LAYERS];                    // K of each GEMM (conv1: padded)
};

static LpipsGeom lpips_geom(int w, int h) {
  LpipsGeom g;
  g.fh[0] = (h - 7) / 4 + 1; g.fw[0] = (w - 7) / 4 + 1;
  g.ph[0] = (g.fh[0] - 3) / 2 + 1; g.pw[0] = (g.fw[0] - 3) / 2 + 1;
  g.fh[1] = g.ph[0]; g.fw[1] = g.pw[0];
  g.ph[1] = (g.fh[1] - 3) / 2 + 1; g.pw[1] = (g.fw[1] - 3) / 2 + 1;
  for (int l = 2; l < LP_LAYERS; ++l) { g.fh[l] = g.ph[1]; g.fw[l] = g.pw[1]; }
  for (int l = 0; l < LP_LAYERS; ++l) {
    g.px[l] = (long)g.fh[l] * g.fw[l];
    g.kp[l] = l == 0 ? LP_K1P : LP_CIN[l] * LP_KS[l] * LP_KS[l];
  }
  return g;
}

struct LpipsLayout {                    // byte offsets into the workspace, each a multiple of 256
  size_t w1p, x, f[LP_LAYERS], pool[2], partial, total;
  long head_blocks, first_block[LP_LAYERS + 1];
};

static LpipsLayout lpips_layout(const LpipsGeom& g) {
  LpipsLayout o;
  size_t at = 0;
  auto take = [&at](size_t bytes) { const size_t here = at; at += (bytes + 255) & ~(size_t)255; return here; };
  o.w1p = take((size_t)LP_COUT[0] * LP_K1P * sizeof(float));
  size_t xmax = 0;
  for (int l = 0; l < LP_LAYERS; ++l) { const size_t n = (size_t)2 * g.px[l] * g.kp[l]; xmax = n > xmax ? n : xmax; }
  o.x = take(xmax * sizeof(float));
  for (int l = 0; l < LP_LAYERS; ++l) o.f[l] = take((size_t)2 * g.px[l] * LP_COUT[l] * sizeof(float));
  for (int l = 0; l < 2; ++l) o.pool[l] = take((size_t)2 * g.ph[l] * g.pw[l] * LP_COUT[l] * sizeof(float));
  o.head_blocks = 0;
  for (int l = 0; l < LP_LAYERS; ++l) { o.first_block[l] = o.head_blocks; o.head_blocks += (g.px[l] + LP_HEAD_PX - 1) / LP_HEAD_PX; }
  o.first_block[LP_LAYERS] = o.head_blocks;
  o.partial = take((size_t)o.head_blocks * sizeof(double));
  o.total = at;
  return o;
}

// X1[m][k] of conv1 (k 11, stride 4, pad 2) straight from the two images, plus the zero-padded copy of its weight rows.
// Element (m, k): image m / (oh ow), output pixel (oy, ox), k = (c, ky, kx) -> ROI pixel (4 oy - 2 + ky, 4 ox - 2 + kx), 0 outside the ROI.
__global__ __launch_bounds__(256) void lpips_patch1_kernel(LpipsArgs a, float* __restrict__ X, float* __restrict__ w1p, int oh, int ow) {
  const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
  const long P = (long)oh * ow, nx = 2 * P * LP_K1P;
  if (idx >= nx) {
    const long j = idx - nx;
    if (j < (long)LP_C1 * LP_K1P) {
      const int n = (int)(j / LP_K1P), k = (int)(j % LP_K1P);
      w1p[j] = k < LP_K1 ? a.conv_w[0][n * LP_K1 + k] : 0.0f;
    }
    return;
  }
  const int k = (int)(idx % LP_K1P);
  const long m = idx / LP_K1P;
  const int img = (int)(m / P), p = (int)(m % P), oy = p / ow, ox = p % ow;
  float v = 0.0f;
  if (k < LP_K1) {
    const int c = k / 121, r = k % 121, ky = r / 11, kx = r % 11;
    const int iy = oy * 4 - 2 + ky, ix = ox * 4 - 2 + kx;
    if (iy >= 0 && iy < a.h && ix >= 0 && ix < a.w) {
      if (img == 0) {
        v = a.pred[(long)c * a.p_sc + (long)(a.y0 + iy) * a.p_sy + (long)(a.x0 + ix) * a.p_sx];
        if (a.quantize_pred) v = truncf(fminf(fmaxf(v, 0.0f), 1.0f) * 255.0f) / 255.0f;   // metrics.hip's expression: eval.py:296-297 + ToTensor
      } else {
        v = a.gt[(long)c * a.g_sc + (long)(a.y0 + iy) * a.g_sy + (long)(a.x0 + ix) * a.g_sx];
      }
      if (a.normalize) v = v * 2.0f - 1.0f;                                              // eval_metric.py:92 / Normalize(.5, .5)
      v = (v - a.shift[c]) / a.scale[c];                                                  // ScalingLayer: a true division
    }
  }
  X[idx] = v;
}

// X[m][k] of a stride-1 convolution over the pixel-major map in[2][H][W][cin]: k = (c, ky, kx), zeros outside the map (same-size output)
__global__ __launch_bounds__(256) void lpips_patch_kernel(const float* __restrict__ in, float* __restrict__ X, int H, int W, int cin, int ks, int pad) {
  const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
  const int K = cin * ks * ks;
  const long P = (long)H * W;
  if (idx >= 2 * P * K) return;
  const int k = (int)(idx % K);
  const long m = idx / K;
  const int img = (int)(m / P), p = (int)(m % P), oy = p / W, ox = p % W;
  const int c = k / (ks * ks), r = k % (ks * ks), ky = r / ks, kx = r % ks;
  const int iy = oy - pad + ky, ix = ox - pad + kx;
  float v = 0.0f;
  if (iy >= 0 && iy < H && ix >= 0 && ix < W) v = in[((long)img * P + (long)iy * W + ix) * cin + c];
  X[idx] = v;
}

// C[m][n] = relu(bias[n] + sum_k A[m][k] B[n][k]); K % 8 == 0, lda / ldb % 4 == 0, A and B 16-byte aligned.  encoder.hip's tile:
// lane (i, kk) loads 16 bytes of row i of A and of B at k = 8 s + 4 kk and issues four MFMAs; wave w owns a fixed range of the K / 8 chunks.
__global__ __launch_bounds__(256) void lpips_gemm_relu_kernel(const float* __restrict__ A, int lda, const float* __restrict__ B, int ldb,
                                                              const float* __restrict__ bias, float* __restrict__ C, int ldc, long M, int N, int K) {
  __shared__ float red[3][16][64];
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int i = lane & 31, kk = lane >> 5;
  const long m0 = (long)blockIdx.x * 32;
  const int n0 = blockIdx.y * 32;
  const long mr = m0 + i < M ? m0 + i : M - 1;                  // clamped rows: always readable, dropped at the store
  const int nr = n0 + i < N ? n0 + i : N - 1;
  const int chunks = K >> 3, q = chunks >> 2, r = chunks & 3;
  const int s0 = wave * q + (wave < r ? wave : r), s1 = s0 + q + (wave < r ? 1 : 0);
  const float* ap = A + mr * lda + 4 * kk;
  const float* bp = B + (long)nr * ldb + 4 * kk;
  lp_f32x16 acc;
#pragma unroll
  for (int e = 0; e < 16; ++e) acc[e] = 0.0f;
  constexpr int U = 4;
  lp_f32x4 a[U], b[U];
  int s = s0;
  for (; s + U <= s1; s += U) {
#pragma unroll
    for (int u = 0; u < U; ++u) { a[u] = *(const lp_f32x4*)(ap + 8 * (s + u)); b[u] = *(const lp_f32x4*)(bp + 8 * (s + u)); }
#pragma unroll
    for (int u = 0; u < U; ++u)
#pragma unroll
      for (int t = 0; t < 4; ++t) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a[u][t], b[u][t], acc, 0, 0, 0);
  }
  for (; s < s1; ++s) {
    const lp_f32x4 av = *(const lp_f32x4*)(ap + 8 * s), bv = *(const lp_f32x4*)(bp + 8 * s);
#pragma unroll
    for (int t = 0; t < 4; ++t) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(av[t], bv[t], acc, 0, 0, 0);
  }
  if (wave > 0) {
#pragma unroll
    for (int e = 0; e < 16; ++e) red[wave - 1][e][lane] = acc[e];
  }
  __syncthreads();
  if (wave == 0) {
    const int n = n0 + i;
    const float bv = n < N ? bias[n] : 0.0f;
#pragma unroll
    for (int e = 0; e < 16; ++e) {
      const long m = m0 + (e & 3) + 8 * (e >> 2) + 4 * kk;           // 32x32 C/D layout: register e of lane (i, kk) = row m, column i
      const float v = bv + (((acc[e] + red[0][e][lane]) + red[1][e][lane]) + red[2][e][lane]);   // fixed order: deterministic
      if (m < M && n < N) C[m * ldc + n] = fmaxf(v, 0.0f);
    }
  }
}

// MaxPool2d(3, 2), floor mode, no padding, on the pixel-major maps of both images: in[2][H][W][C] -> out[2][Ho][Wo][C]
__global__ __launch_bounds__(256) void lpips_pool_kernel(const float* __restrict__ in, float* __restrict__ out, int H, int W, int C, int Ho, int Wo) {
  const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= 2L * Ho * Wo * C) return;
  const int c = (int)(idx % C);
  const long q = idx / C;
  const int img = (int)(q / ((long)Ho * Wo)), p = (int)(q % ((long)Ho * Wo)), y = p / Wo, x = p % Wo;
  const float* s = in + (((long)img * H + 2 * y) * W + 2 * x) * C + c;     // rows 2y .. 2y+2 <= H-1, columns 2x .. 2x+2 <= W-1 by Ho, Wo
  float v = s[0];
#pragma unroll
  for (int dy = 0; dy < 3; ++dy)
#pragma unroll
    for (int dx = 0; dx < 3; ++dx) v = fmaxf(v, s[((long)dy * W + dx) * C]);
  out[idx] = v;
}

// the pixel-major map F[2][P][C] as the two [C][P] (= [C,h,w]) tensors a caller asked for
__global__ __launch_bounds__(256) void lpips_features_kernel(const float* __restrict__ F, float* __restrict__ out0, float* __restrict__ out1, long P, int C) {
  const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= 2 * P * C) return;
  const int img = (int)(idx / (P * C));
  const long j = idx % (P * C), c = j / P, p = j % P;
  (img ? out1 : out0)[j] = F[((long)img * P + p) * C + c];
}

struct LpipsHeadArgs {
  const float* F[LP_LAYERS];
  const float* lin[LP_LAYERS];
  long P[LP_LAYERS];
  int C[LP_LAYERS];
  long first_block[LP_LAYERS + 1];
};

// One wave = one pixel at a time: lane j holds channels j, j + 64, ... (C <= 384) of both images; s = sum_c F^2 per image (xor tree over
// the lanes), n = F / (sqrt(s) + 1e-10), d = sum_c lin[c] (n0 - n1)^2.  Wave w of a workgroup takes pixels w, w + 4, w + 8, w + 12 of the
// workgroup's 16 and adds their d in double; partial[block] = the four waves in index order.
__global__ __launch_bounds__(256) void lpips_head_kernel(LpipsHeadArgs a, double* __restrict__ partial) {
  __shared__ double red[4];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const long blk = blockIdx.x;
  int l = 0;
#pragma unroll
  for (int j = 1; j < LP_LAYERS; ++j) l += blk >= a.first_block[j] ? 1 : 0;
  const int C = a.C[l], nch = C / 64;
  const long P = a.P[l], p0 = (blk - a.first_block[l]) * LP_HEAD_PX;
  const float* __restrict__ F = a.F[l];
  const float* __restrict__ lin = a.lin[l];
  double acc = 0.0;
  for (int j = 0; j < LP_HEAD_PX / 4; ++j) {
    const long p = p0 + wave + 4 * j;
    if (p >= P) break;
    const float* f0 = F + p * C;
    const float* f1 = F + (P + p) * C;
    float v0[6], v1[6], s0 = 0.0f, s1 = 0.0f;
#pragma unroll
    for (int t = 0; t < 6; ++t) {
      v0[t] = t < nch ? f0[lane + 64 * t] : 0.0f;
      v1[t] = t < nch ? f1[lane + 64 * t] : 0.0f;
      s0 = fmaf(v0[t], v0[t], s0); s1 = fmaf(v1[t], v1[t], s1);
    }
#pragma unroll
    for (int s = 32; s >= 1; s >>= 1) { s0 += __shfl_xor(s0, s); s1 += __shfl_xor(s1, s); }
    const float r0 = sqrtf(s0) + LP_EPS, r1 = sqrtf(s1) + LP_EPS;
    float d = 0.0f;
#pragma unroll
    for (int t = 0; t < 6; ++t) {
      if (t < nch) {
        const float df = v0[t] / r0 - v1[t] / r1;
        d = fmaf(lin[lane + 64 * t], df * df, d);
      }
    }
#pragma unroll
    for (int s = 32; s >= 1; s >>= 1) d += __shfl_xor(d, s);
    acc += (double)d;
  }
  if (lane == 0) red[wave] = acc;
  __syncthreads();
  if (threadIdx.x == 0) partial[blk] = ((red[0] + red[1]) + red[2]) + red[3];
}

// one workgroup: per layer, thread t adds partial[first + t], partial[first + t + 256], ... in that order, then a fixed LDS tree;
// out6 = {d_1 .. d_5 (means over the layer's pixels), their sum added in layer order}
__global__ __launch_bounds__(256) void lpips_final_kernel(const double* __restrict__ partial, LpipsHeadArgs a, double* __restrict__ out6) {
  __shared__ double red[256];
  double total = 0.0;
  for (int l = 0; l < LP_LAYERS; ++l) {
    double s = 0.0;
    for (long b = a.first_block[l] + threadIdx.x; b < a.first_block[l + 1]; b += 256) s += partial[b];
    red[threadIdx.x] = s;
    __syncthreads();
    for (int h = 128; h >= 1; h >>= 1) {
      if ((int)threadIdx.x < h) red[threadIdx.x] += red[threadIdx.x + h];
      __syncthreads();
    }
    const double d = red[0] / (double)a.P[l];
    __syncthreads();
    if (threadIdx.x == 0) out6[l] = d;
    total += d;
  }
  if (threadIdx.x == 0) out6[LP_LAYERS] = total;
}

size_t lpips_workspace_bytes(int w, int h) { return lpips_layout(lpips_geom(w, h)).total; }

bool lpips_fits_one_launch(int w, int h) {
  const LpipsGeom g = lpips_geom(w, h);
  long most = 0;
  for (int l = 0; l < LP_LAYERS; ++l) { const long n = (2 * g.px[l] * g.kp[l] + (long)LP_C1 * LP_K1P) / 256 + 1; most = n > most ? n : most; }
  return most <= 0x7fffffffL;        // blocks of the widest launch (the patch matrices)
}

static inline unsigned lp_blocks(long n) { return (unsigned)((n + 255) / 256); }

int launch_lpips(const LpipsArgs& a, double* out6, float* const* features, void* workspace, hipStream_t stream) {
  const LpipsGeom g = lpips_geom(a.w, a.h);
  const LpipsLayout o = lpips_layout(g);
  char* ws = (char*)workspace;
  float* w1p = (float*)(ws + o.w1p);
  float* X = (float*)(ws + o.x);
  float* F[LP_LAYERS];
  for (int l = 0; l < LP_LAYERS; ++l) F[l] = (float*)(ws + o.f[l]);
  float* pool[2] = {(float*)(ws + o.pool[0]), (float*)(ws + o.pool[1])};
  double* partial = (double*)(ws + o.partial);

  for (int l = 0; l < LP_LAYERS; ++l) {
    const long M = 2 * g.px[l];
    const float* B = a.conv_w[l];
    if (l == 0) {
      hipLaunchKernelGGL(lpips_patch1_kernel, dim3(lp_blocks(M * LP_K1P + (long)LP_COUT[0] * LP_K1P)), dim3(256), 0, stream, a, X, w1p, g.fh[0], g.fw[0]);
      B = w1p;
    } else {
      const float* in = F[l - 1];
      if (l <= 2) {       // conv2 and conv3 read the pooled map
        hipLaunchKernelGGL(lpips_pool_kernel, dim3(lp_blocks(2L * g.ph[l - 1] * g.pw[l - 1] * LP_COUT[l - 1])), dim3(256), 0, stream,
                           (const float*)F[l - 1], pool[l - 1], g.fh[l - 1], g.fw[l - 1], LP_COUT[l - 1], g.ph[l - 1], g.pw[l - 1]);
        in = pool[l - 1];
      }
      hipLaunchKernelGGL(lpips_patch_kernel, dim3(lp_blocks(M * g.kp[l])), dim3(256), 0, stream, in, X, g.fh[l], g.fw[l], LP_CIN[l], LP_KS[l], LP_PAD[l]);
    }
    hipLaunchKernelGGL(lpips_gemm_relu_kernel, dim3((unsigned)((M + 31) / 32), (unsigned)(LP_COUT[l] / 32)), dim3(256), 0, stream,
                       (const float*)X, g.kp[l], B, g.kp[l], a.conv_b[l], F[l], LP_COUT[l], M, LP_COUT[l], g.kp[l]);
    if (features)
      hipLaunchKernelGGL(lpips_features_kernel, dim3(lp_blocks(M * LP_COUT[l])), dim3(256), 0, stream, (const float*)F[l], features[l],
                         features[LP_LAYERS + l], g.px[l], LP_COUT[l]);
  }
  LpipsHeadArgs ha;
  for (int l = 0; l < LP_LAYERS; ++l) { ha.F[l] = F[l]; ha.lin[l] = a.lin[l]; ha.P[l] = g.px[l]; ha.C[l] = LP_COUT[l]; ha.first_block[l] = o.first_block[l]; }
  ha.first_block[LP_LAYERS] = o.first_block[LP_LAYERS];
  hipLaunchKernelGGL(lpips_head_kernel, dim3((unsigned)o.head_blocks), dim3(256), 0, stream, ha, partial);
  hipLaunchKernelGGL(lpips_final_kernel, dim3(1), dim3(256), 0, stream, (const double*)partial, ha, out6);
  return check_launch("lpips");
}

}  // namespace crnerf

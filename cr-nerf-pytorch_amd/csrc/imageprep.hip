// Image preparation: Pillow's 8-bit LANCZOS resize of a decoded photo, bit for bit, with torchvision's
// ToTensor / Normalize(0.5, 0.5) fused into the store of the last pass that runs.
//
// Reference: PIL.Image.resize((w, h), Image.LANCZOS) followed by T.ToTensor() and optionally T.Normalize(0.5, 0.5), as
//            datasets/phototourism_mask_grid_sample.py:183-199 / :288-320 and eval.py:140-151 build rgbs, whole_img and the style image.
// Pillow's arithmetic, restated (include/crnerf.h carries the definition): per axis a table of 22-bit fixed-point coefficients
// k[out][ksize] and windows (xmin, xmax), built on the host in float64; one pass is acc = 2^21 + sum in[xmin + x] * k[x] in int32,
// out = clamp(acc >> 22, 0, 255); the horizontal pass runs first into a uint8 image, the vertical pass second; a pass that keeps its
// size is skipped.  Integer arithmetic: no order of summation matters, the result is Pillow's byte.
// No roofline is claimed: a 1400x2000 photo is 8.4 MB of reads, the two launches dominate below that.
#include <hip/hip_runtime.h>
#include "kernels.h"

namespace crnerf {

constexpr int LZ_THREADS = 256;
constexpr int LZ_BITS = 22;                                   // Pillow's PRECISION_BITS
static_assert(LANCZOS_TILE_W * LANCZOS_TILE_H == LZ_THREADS, "horizontal pass: one thread per pixel of the tile");
static_assert(LANCZOS_VBLOCK == LZ_THREADS, "vertical pass: one thread per byte of the block's row piece");

struct LanczosOut {
  void* dst;
  int mode;          // LANCZOS_U8 ... LANCZOS_CHW_SIGNED
  int w;             // output row length in pixels
  long plane;        // h * w (the channel stride of the chw modes)
};

__device__ __forceinline__ int lz_round(int acc) { return min(max(acc >> LZ_BITS, 0), 255); }   // arithmetic shift

// byte v of channel c of output pixel (y, x)
__device__ __forceinline__ void lz_store(const LanczosOut& o, int y, int x, int c, int v) {
  const long p = (long)y * o.w + x;
  if (o.mode == LANCZOS_U8) { ((uint8_t*)o.dst)[p * 3 + c] = (uint8_t)v; return; }
  float f = (float)v / 255.0f;                                // ToTensor: a true (correctly rounded) division
  if (o.mode == LANCZOS_ROWS) { ((float*)o.dst)[p * 3 + c] = f; return; }
  if (o.mode == LANCZOS_CHW_SIGNED) f = (f - 0.5f) / 0.5f;    // Normalize(0.5, 0.5)
  ((float*)o.dst)[(long)c * o.plane + p] = f;
}

// Horizontal pass.  One workgroup = LANCZOS_TILE_H rows x LANCZOS_TILE_W output columns.  Dynamic LDS: the tile's coefficient rows
// [ncols][ksize] (copied 16 bytes at a time: a tile's rows start 16-byte aligned in the table), then per row the input bytes the tile's
// windows cover, [LANCZOS_TILE_H][pitch], copied in 16-byte pieces aligned in GLOBAL memory (row r's segment starts `head(r)` bytes
// into its LDS row).  Lanes of a wave are 32 columns x 2 rows: the coefficient reads of a tap are ksize dwords apart (ksize is odd: no
// bank conflict), the two rows broadcast.
// Whatever the tables hold, nothing outside the source, the tables and the LDS rows is touched: windows are clamped to the tile's span.
__global__ __launch_bounds__(LZ_THREADS) void lanczos_horizontal_kernel(const uint8_t* __restrict__ src, int H, int W, int w,
                                                                        const int* __restrict__ kx, const int* __restrict__ bx, int ksize,
                                                                        int pitch, LanczosOut out) {
  extern __shared__ int4 lz_lds[];
  int* sk = (int*)lz_lds;
  const int x0 = blockIdx.x * LANCZOS_TILE_W, y0 = blockIdx.y * LANCZOS_TILE_H;
  const int ncols = min(LANCZOS_TILE_W, w - x0), nrows = min(LANCZOS_TILE_H, H - y0);
  uint8_t* sin = (uint8_t*)(sk + ((LANCZOS_TILE_W * ksize + 3) & ~3));
  // the tile's span of input pixels [lo, hi): windows move right with the column
  const int lo = min(max(bx[2 * x0], 0), W);
  const int last = x0 + ncols - 1;
  int hi = min(max(bx[2 * last] + bx[2 * last + 1], lo), W);
  hi = min(hi, lo + (pitch - 16) / 3);
  const long rb = (long)W * 3;
  const uintptr_t g_begin = (uintptr_t)src, g_end = g_begin + (size_t)H * rb;

  const int nk = ncols * ksize;
  const int* kt = kx + (long)x0 * ksize;
  for (int i = threadIdx.x; i < nk / 4; i += LZ_THREADS) ((int4*)sk)[i] = ((const int4*)kt)[i];
  for (int i = (nk & ~3) + threadIdx.x; i < nk; i += LZ_THREADS) sk[i] = kt[i];

  const int seg = (hi - lo) * 3;                              // bytes of a row's segment
  const int nch = (seg + 15 + 15) / 16;                       // 16-byte pieces, for any head
  for (int i = threadIdx.x; i < nrows * nch; i += LZ_THREADS) {
    const int r = i / nch, ch = i - r * nch;
    const uintptr_t g0 = g_begin + (size_t)(y0 + r) * rb + (size_t)lo * 3;
    const int head = (int)(g0 & 15);
    if (ch * 16 >= head + seg) continue;
    const uintptr_t g = g0 - head + (size_t)ch * 16;
    uint8_t* d = sin + r * pitch + ch * 16;
    if (g >= g_begin && g + 16 <= g_end) {
      *(int4*)d = *(const int4*)g;
    } else {                                                  // the piece hangs over the first or the last byte of the image
      for (int b = 0; b < 16; ++b)
        if (g + b >= g_begin && g + b < g_end) d[b] = *(const uint8_t*)(g + b);
    }
  }
  __syncthreads();

  const int col = threadIdx.x % LANCZOS_TILE_W, row = threadIdx.x / LANCZOS_TILE_W;
  if (col >= ncols || row >= nrows) return;
  const int x = x0 + col, y = y0 + row;
  const int xmin = min(max(bx[2 * x], lo), hi);
  const int xmax = min(min(max(bx[2 * x + 1], 0), ksize), hi - xmin);
  const int head = (int)((g_begin + (size_t)y * rb + (size_t)lo * 3) & 15);
  const uint8_t* p = sin + row * pitch + head + (xmin - lo) * 3;
  const int* k = sk + col * ksize;
  int a0 = 1 << (LZ_BITS - 1), a1 = a0, a2 = a0;
  for (int t = 0; t < xmax; ++t) {
    const int kk = k[t];
    a0 += (int)p[3 * t] * kk; a1 += (int)p[3 * t + 1] * kk; a2 += (int)p[3 * t + 2] * kk;
  }
  lz_store(out, y, x, 0, lz_round(a0));
  lz_store(out, y, x, 1, lz_round(a1));
  lz_store(out, y, x, 2, lz_round(a2));
}

// Vertical pass.  One workgroup = LANCZOS_VBLOCK consecutive bytes of one output row: consecutive lanes read consecutive bytes of every
// input row of the window, the coefficient row is uniform over the workgroup.  in: [H, w, 3] uint8 (the source itself when the
// horizontal pass is skipped).
__global__ __launch_bounds__(LZ_THREADS) void lanczos_vertical_kernel(const uint8_t* __restrict__ in, int H, int w, const int* __restrict__ ky,
                                                                      const int* __restrict__ by, int ksize, LanczosOut out) {
  const int rb = w * 3;
  const int b = blockIdx.x * LANCZOS_VBLOCK + threadIdx.x, y = blockIdx.y;
  if (b >= rb) return;
  const int ymin = min(max(by[2 * y], 0), H);
  const int ymax = min(min(max(by[2 * y + 1], 0), ksize), H - ymin);
  const int* k = ky + (long)y * ksize;
  const uint8_t* p = in + (long)ymin * rb + b;
  int acc = 1 << (LZ_BITS - 1);
  for (int t = 0; t < ymax; ++t) acc += (int)p[(long)t * rb] * k[t];
  const int x = b / 3;
  lz_store(out, y, x, b - 3 * x, lz_round(acc));
}

// Neither pass runs (w == W, h == H): the conversions alone.
__global__ __launch_bounds__(LZ_THREADS) void lanczos_convert_kernel(const uint8_t* __restrict__ src, long n_bytes, LanczosOut out) {
  const long i = (long)blockIdx.x * LZ_THREADS + threadIdx.x;
  if (i >= n_bytes) return;
  const long p = i / 3;
  lz_store(out, (int)(p / out.w), (int)(p % out.w), (int)(i - 3 * p), src[i]);
}

int lanczos_ksize(int in_size, int out_size) {
  const double scale = (double)in_size / (double)out_size, fs = scale > 1.0 ? scale : 1.0;
  return (int)ceil(3.0 * fs) * 2 + 1;
}

size_t lanczos_workspace_bytes(int H, int W, int w, int h) { return (w != W && h != H) ? (size_t)H * w * 3 : 0; }

// LDS of the horizontal pass: the tile's coefficients and LANCZOS_TILE_H row segments.  A tile's windows span at most
// (TILE_W - 1) * scale + 1 pixels between the first and the last xmin, plus ksize; each row carries up to 15 bytes of head and is padded to 16.
static void lanczos_horizontal_lds(int W, int w, int ksize, int* pitch, size_t* bytes) {
  long span = (long)((double)(LANCZOS_TILE_W - 1) * ((double)W / (double)w)) + 2 + ksize;
  if (span > W) span = W;
  *pitch = (int)((span * 3 + 15 + 15) / 16 * 16) + 16;
  *bytes = (size_t)((LANCZOS_TILE_W * ksize + 3) & ~3) * sizeof(int) + (size_t)LANCZOS_TILE_H * *pitch;
}

bool lanczos_fits(int H, int W, int w, int h) {
  if ((long)H * W * 3 > 0x7fffffffL || (long)h * w * 3 > 0x7fffffffL || (long)H * w * 3 > 0x7fffffffL) return false;
  if (w != W) {
    int pitch; size_t bytes;
    lanczos_horizontal_lds(W, w, lanczos_ksize(W, w), &pitch, &bytes);
    if (bytes > 64 * 1024) return false;
  }
  return (H + LANCZOS_TILE_H - 1) / LANCZOS_TILE_H <= 65535 && h <= 65535;      // grid y
}

int launch_lanczos_resize(const uint8_t* src, int H, int W, int w, int h, const int* kx, const int* bx, int ksize_x, const int* ky, const int* by,
                          int ksize_y, int mode, void* dst, void* workspace, hipStream_t stream) {
  const LanczosOut final_out{dst, mode, w, (long)h * w};
  const bool horiz = w != W, vert = h != H;
  if (!horiz && !vert) {
    const long n = (long)H * W * 3;
    hipLaunchKernelGGL(lanczos_convert_kernel, dim3((unsigned)((n + LZ_THREADS - 1) / LZ_THREADS)), dim3(LZ_THREADS), 0, stream, src, n, final_out);
    return check_launch("lanczos_convert");
  }
  const uint8_t* vin = src;
  if (horiz) {
    int pitch; size_t lds;
    lanczos_horizontal_lds(W, w, ksize_x, &pitch, &lds);
    const LanczosOut mid{workspace, LANCZOS_U8, w, (long)H * w};
    const dim3 grid((unsigned)((w + LANCZOS_TILE_W - 1) / LANCZOS_TILE_W), (unsigned)((H + LANCZOS_TILE_H - 1) / LANCZOS_TILE_H));
    hipLaunchKernelGGL(lanczos_horizontal_kernel, grid, dim3(LZ_THREADS), lds, stream, src, H, W, w, kx, bx, ksize_x, pitch, vert ? mid : final_out);
    vin = (const uint8_t*)workspace;
  }
  if (vert) {
    const dim3 grid((unsigned)((w * 3 + LANCZOS_VBLOCK - 1) / LANCZOS_VBLOCK), (unsigned)h);
    hipLaunchKernelGGL(lanczos_vertical_kernel, grid, dim3(LZ_THREADS), 0, stream, vin, H, w, ky, by, ksize_y, final_out);
  }
  return check_launch("lanczos_resize");
}

}  // namespace crnerf

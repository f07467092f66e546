// RGBA preparation: one chain for a decoded Blender frame, uint8 [H, W, 4], one dword per pixel -- the occluder rectangles
// and the colour table of add_perturbation, Pillow's LANCZOS resize of an RGBA image (through its premultiplied mode RGBa), and the white
// blend / ToTensor / Normalize of the dataset fused into the store of the last pass that runs.
//
// Reference: datasets/blender_mask_grid_sample.py:16-36 (add_perturbation), :106-110 and :174-178 (resize, toTensor, blend), eval.py:99-111.
// The arithmetic is stated in include/crnerf_blender.h.  Load stage (in whichever pass reads the source): the last rectangle that holds the
// pixel replaces it with (colour, alpha 255); the table maps R, G, B; with a resize, c' = MULDIV255(c, a).  The passes are those of
// imageprep.hip on four channels: int32 accumulator from 2^21, arithmetic shift by 22, clamp, horizontal first, uint8 in between.  Store
// stage: with a resize, c = min(255, 255 c' / a) for 0 < a < 255; then the dword, or x = c/255, a = alpha/255, x*a + (1 - a), each
// operation rounded on its own (no contraction: see the pragma below and -ffp-contract=off of the build).
// Integer arithmetic up to the store: no order of summation matters.  No roofline is claimed; profiles/r13/blender_prep.txt has the timings.
#include <hip/hip_runtime.h>
#include "kernels.h"

#pragma clang fp contract(off)

namespace crnerf {

constexpr int RG_THREADS = 256;
constexpr int RG_BITS = 22;                                   // Pillow's PRECISION_BITS
static_assert(RGBA_TILE_W * RGBA_TILE_H == RG_THREADS, "horizontal pass: one thread per pixel of the tile");
static_assert(RGBA_VBLOCK == RG_THREADS, "vertical pass: one thread per pixel of the block's row piece");
static_assert(RGBA_MAX_RECTS <= 32, "the candidate rectangles of a pixel are one 32-bit mask");

struct RgbaLoad {
  int n_rects;
  int rect[RGBA_MAX_RECTS][4];      // inclusive x0, y0, x1, y1
  uint32_t color[RGBA_MAX_RECTS];   // the rectangle's pixel: R | G << 8 | B << 16 | 255 << 24
  const uint8_t* lut;               // [3][256] or null
  int premul;                       // a resize follows: store premultiplied colour
};

struct RgbaOut {
  void* dst;
  uint8_t* valid;    // [h * w] = alpha > 0, or null
  int mode;          // RGBA_U8 ... RGBA_CHW_SIGNED
  int w;             // output row length in pixels
  long plane;        // h * w (the channel stride of the chw modes)
  int unpremul;      // a resize ran: the colour is premultiplied
};

__device__ __forceinline__ int rg_round(int acc) { return min(max(acc >> RG_BITS, 0), 255); }   // arithmetic shift
__device__ __forceinline__ uint32_t rg_muldiv255(uint32_t c, uint32_t a) {                      // Pillow's MULDIV255
  const uint32_t t = c * a + 128u;
  return ((t >> 8) + t) >> 8;
}

// the colour table into LDS; every thread of the workgroup calls it, a barrier follows
__device__ __forceinline__ void rg_stage_lut(const RgbaLoad& ld, uint8_t* slut) {
  if (ld.lut)
    for (int i = threadIdx.x; i < 768; i += RG_THREADS) slut[i] = ld.lut[i];
}

// rectangles whose x range holds column x
__device__ __forceinline__ uint32_t rg_column_mask(const RgbaLoad& ld, int x) {
  uint32_t m = 0;
  for (int i = 0; i < ld.n_rects; ++i)
    if (x >= ld.rect[i][0] && x <= ld.rect[i][2]) m |= 1u << i;
  return m;
}

// source pixel (y, x) after the load stage; mask: the rectangles that may hold it
__device__ __forceinline__ uint32_t rg_load(uint32_t px, int y, uint32_t mask, const RgbaLoad& ld, const uint8_t* slut) {
  while (mask) {
    const int i = 31 - __clz((int)mask);                      // the last rectangle wins
    if (y >= ld.rect[i][1] && y <= ld.rect[i][3]) { px = ld.color[i]; break; }
    mask &= ~(1u << i);
  }
  uint32_t r = px & 255u, g = (px >> 8) & 255u, b = (px >> 16) & 255u;
  const uint32_t a = px >> 24;
  if (ld.lut) { r = slut[r]; g = slut[256 + g]; b = slut[512 + b]; }
  if (ld.premul) { r = rg_muldiv255(r, a); g = rg_muldiv255(g, a); b = rg_muldiv255(b, a); }
  return r | (g << 8) | (b << 16) | (a << 24);
}

// output pixel (y, x) = (r, g, b, a), each in [0, 255]
__device__ __forceinline__ void rg_store(const RgbaOut& o, int y, int x, int r, int g, int b, int a) {
  const long p = (long)y * o.w + x;
  if (o.unpremul && a != 0 && a != 255) {                     // Pillow's rgbA2rgba
    r = min(255, 255 * r / a); g = min(255, 255 * g / a); b = min(255, 255 * b / a);
  }
  if (o.valid) o.valid[p] = (uint8_t)(a > 0);
  if (o.mode == RGBA_U8) { ((uint32_t*)o.dst)[p] = (uint32_t)r | ((uint32_t)g << 8) | ((uint32_t)b << 16) | ((uint32_t)a << 24); return; }
  const float fa = (float)a / 255.0f, ia = 1.0f - fa;         // ToTensor: true divisions; img[:3] * img[-1:] + (1 - img[-1:])
  float f[3] = {(float)r / 255.0f, (float)g / 255.0f, (float)b / 255.0f};
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const float m = f[c] * fa;
    f[c] = m + ia;
  }
  float* d = (float*)o.dst;
  if (o.mode == RGBA_ROWS) { d[p * 3] = f[0]; d[p * 3 + 1] = f[1]; d[p * 3 + 2] = f[2]; return; }
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const float v = o.mode == RGBA_CHW_SIGNED ? (f[c] - 0.5f) / 0.5f : f[c];   // Normalize(0.5, 0.5)
    d[(long)c * o.plane + p] = v;
  }
}

// Horizontal pass.  One workgroup = RGBA_TILE_H rows x RGBA_TILE_W output columns.  Dynamic LDS: the tile's coefficient rows [ncols][ksize]
// (a tile's rows start 16-byte aligned in the table), then per row the pixels the tile's windows cover after the load stage, one dword
// each, [RGBA_TILE_H][pitch] with pitch odd.  Whatever the tables hold, nothing outside the source, the tables and the LDS rows is touched:
// windows are clamped to the tile's span, the span to the row and to pitch.
__global__ __launch_bounds__(RG_THREADS) void rgba_horizontal_kernel(const uint32_t* __restrict__ src, int H, int W, int w, const int* __restrict__ kx,
                                                                     const int* __restrict__ bx, int ksize, int pitch, RgbaLoad ld, RgbaOut out) {
  extern __shared__ int4 rg_lds[];
  __shared__ uint8_t slut[768];
  int* sk = (int*)rg_lds;
  uint32_t* sin = (uint32_t*)(sk + ((RGBA_TILE_W * ksize + 3) & ~3));
  const int x0 = blockIdx.x * RGBA_TILE_W, y0 = blockIdx.y * RGBA_TILE_H;
  const int ncols = min(RGBA_TILE_W, w - x0), nrows = min(RGBA_TILE_H, H - y0);
  // the tile's span of input pixels [lo, hi): windows move right with the column
  const int lo = min(max(bx[2 * x0], 0), W);
  const int last = x0 + ncols - 1;
  int hi = min(max(bx[2 * last] + bx[2 * last + 1], lo), W);
  hi = min(hi, lo + pitch);
  const int span = hi - lo;

  rg_stage_lut(ld, slut);
  const int nk = ncols * ksize;
  const int* kt = kx + (long)x0 * ksize;
  for (int i = threadIdx.x; i < nk / 4; i += RG_THREADS) ((int4*)sk)[i] = ((const int4*)kt)[i];
  for (int i = (nk & ~3) + threadIdx.x; i < nk; i += RG_THREADS) sk[i] = kt[i];
  __syncthreads();

  const uint32_t every = ld.n_rects >= 32 ? ~0u : (1u << ld.n_rects) - 1u;
  for (int i = threadIdx.x; i < nrows * span; i += RG_THREADS) {
    const int r = i / span, c = i - r * span;
    const int x = lo + c, y = y0 + r;
    uint32_t m = every;
    if (m) m = rg_column_mask(ld, x);
    sin[r * pitch + c] = rg_load(src[(long)y * W + x], y, m, ld, slut);
  }
  __syncthreads();

  const int col = threadIdx.x % RGBA_TILE_W, row = threadIdx.x / RGBA_TILE_W;
  if (col >= ncols || row >= nrows) return;
  const int x = x0 + col, y = y0 + row;
  const int xmin = min(max(bx[2 * x], lo), hi);
  const int xmax = min(min(max(bx[2 * x + 1], 0), ksize), hi - xmin);
  const uint32_t* p = sin + row * pitch + (xmin - lo);
  const int* k = sk + col * ksize;
  int a0 = 1 << (RG_BITS - 1), a1 = a0, a2 = a0, a3 = a0;
  for (int t = 0; t < xmax; ++t) {
    const int kk = k[t];
    const uint32_t px = p[t];
    a0 += (int)(px & 255u) * kk; a1 += (int)((px >> 8) & 255u) * kk; a2 += (int)((px >> 16) & 255u) * kk; a3 += (int)(px >> 24) * kk;
  }
  rg_store(out, y, x, rg_round(a0), rg_round(a1), rg_round(a2), rg_round(a3));
}

// Vertical pass.  One workgroup = RGBA_VBLOCK consecutive pixels of one output row: consecutive lanes read consecutive dwords of every
// input row of the window, the coefficient row is uniform over the workgroup.  in: [H, w] dwords -- the premultiplied image of the
// horizontal pass (ld then does nothing), or the source itself when that pass is skipped (ld is the load stage).
__global__ __launch_bounds__(RG_THREADS) void rgba_vertical_kernel(const uint32_t* __restrict__ in, int H, int w, const int* __restrict__ ky,
                                                                   const int* __restrict__ by, int ksize, RgbaLoad ld, RgbaOut out) {
  __shared__ uint8_t slut[768];
  rg_stage_lut(ld, slut);
  __syncthreads();
  const int x = blockIdx.x * RGBA_VBLOCK + threadIdx.x, y = blockIdx.y;
  if (x >= w) return;
  const int ymin = min(max(by[2 * y], 0), H);
  const int ymax = min(min(max(by[2 * y + 1], 0), ksize), H - ymin);
  const int* k = ky + (long)y * ksize;
  const uint32_t* p = in + (long)ymin * w + x;
  const bool staged = ld.n_rects > 0 || ld.lut != nullptr || ld.premul;
  const uint32_t m = rg_column_mask(ld, x);
  int a0 = 1 << (RG_BITS - 1), a1 = a0, a2 = a0, a3 = a0;
  for (int t = 0; t < ymax; ++t) {
    const int kk = k[t];
    uint32_t px = p[(long)t * w];
    if (staged) px = rg_load(px, ymin + t, m, ld, slut);
    a0 += (int)(px & 255u) * kk; a1 += (int)((px >> 8) & 255u) * kk; a2 += (int)((px >> 16) & 255u) * kk; a3 += (int)(px >> 24) * kk;
  }
  rg_store(out, y, x, rg_round(a0), rg_round(a1), rg_round(a2), rg_round(a3));
}

// Neither pass runs (w == W, h == H): the load stage without the premultiply, and the store.
__global__ __launch_bounds__(RG_THREADS) void rgba_convert_kernel(const uint32_t* __restrict__ src, long n_pixels, RgbaLoad ld, RgbaOut out) {
  __shared__ uint8_t slut[768];
  rg_stage_lut(ld, slut);
  __syncthreads();
  const long i = (long)blockIdx.x * RG_THREADS + threadIdx.x;
  if (i >= n_pixels) return;
  const int y = (int)(i / out.w), x = (int)(i - (long)y * out.w);
  const uint32_t px = rg_load(src[i], y, rg_column_mask(ld, x), ld, slut);
  rg_store(out, y, x, (int)(px & 255u), (int)((px >> 8) & 255u), (int)((px >> 16) & 255u), (int)(px >> 24));
}

size_t rgba_workspace_bytes(int H, int W, int w, int h) { return (w != W && h != H) ? (size_t)H * w * 4 : 0; }

// LDS of the horizontal pass: the tile's coefficients and RGBA_TILE_H row segments of `pitch` dwords.  A tile's windows span at most
// (TILE_W - 1) * scale + 1 pixels between the first and the last xmin, plus ksize.
static void rgba_horizontal_lds(int W, int w, int ksize, int* pitch, size_t* bytes) {
  long span = (long)((double)(RGBA_TILE_W - 1) * ((double)W / (double)w)) + 2 + ksize;
  if (span > W) span = W;
  *pitch = (int)span | 1;
  *bytes = (size_t)((RGBA_TILE_W * ksize + 3) & ~3) * sizeof(int) + (size_t)RGBA_TILE_H * *pitch * sizeof(uint32_t);
}

bool rgba_fits(int H, int W, int w, int h) {
  if ((long)H * W * 4 > 0x7fffffffL || (long)h * w * 4 > 0x7fffffffL || (long)H * w * 4 > 0x7fffffffL) return false;
  if (w != W) {
    int pitch; size_t bytes;
    rgba_horizontal_lds(W, w, lanczos_ksize(W, w), &pitch, &bytes);
    if (bytes > 64 * 1024) return false;
  }
  return (H + RGBA_TILE_H - 1) / RGBA_TILE_H <= 65535 && h <= 65535;      // grid y
}

int launch_rgba_prepare(const RgbaPrepare& a, hipStream_t stream) {
  const bool horiz = a.w != a.W, vert = a.h != a.H, resize = horiz || vert;
  RgbaLoad first{};                                           // the load stage, in whichever pass reads the source
  first.n_rects = a.n_rects;
  for (int i = 0; i < a.n_rects; ++i) {
    for (int c = 0; c < 4; ++c) first.rect[i][c] = a.rects[4 * i + c];
    first.color[i] = (uint32_t)a.colors[3 * i] | ((uint32_t)a.colors[3 * i + 1] << 8) | ((uint32_t)a.colors[3 * i + 2] << 16) | 0xff000000u;
  }
  first.lut = a.lut;
  first.premul = resize ? 1 : 0;
  const RgbaLoad none{};
  const RgbaOut final_out{a.dst, a.valid, a.mode, a.w, (long)a.h * a.w, resize ? 1 : 0};
  const uint32_t* src = (const uint32_t*)a.src;
  if (!resize) {
    const long n = (long)a.H * a.W;
    hipLaunchKernelGGL(rgba_convert_kernel, dim3((unsigned)((n + RG_THREADS - 1) / RG_THREADS)), dim3(RG_THREADS), 0, stream, src, n, first, final_out);
    return check_launch("rgba_convert");
  }
  const uint32_t* vin = src;
  if (horiz) {
    int pitch; size_t lds;
    rgba_horizontal_lds(a.W, a.w, a.ksize_x, &pitch, &lds);
    const RgbaOut mid{a.workspace, nullptr, RGBA_U8, a.w, (long)a.H * a.w, 0};
    const dim3 grid((unsigned)((a.w + RGBA_TILE_W - 1) / RGBA_TILE_W), (unsigned)((a.H + RGBA_TILE_H - 1) / RGBA_TILE_H));
    hipLaunchKernelGGL(rgba_horizontal_kernel, grid, dim3(RG_THREADS), lds, stream, src, a.H, a.W, a.w, a.kx, a.bx, a.ksize_x, pitch, first,
                       vert ? mid : final_out);
    vin = (const uint32_t*)a.workspace;
  }
  if (vert) {
    const dim3 grid((unsigned)((a.w + RGBA_VBLOCK - 1) / RGBA_VBLOCK), (unsigned)a.h);
    hipLaunchKernelGGL(rgba_vertical_kernel, grid, dim3(RG_THREADS), 0, stream, vin, a.H, a.w, a.ky, a.by, a.ksize_y, horiz ? none : first, final_out);
  }
  return check_launch("rgba_prepare");
}

}  // namespace crnerf

// Backward-data pass of NeRF_sigma on the x3 core (mlp_core_x3.h): mlp_backward16_kernel's job (mlp_train16.hip) -- the layer deltas
//   delta_{l-1} = (W_l^T delta_l) . relu'(h_{l-1})          (in the reference: PyTorch autograd over the addmm nodes of models/nerf.py:157-182)
// -- with every product formed from three-piece bf16 splits on the bf16 matrix cores (fp32-accurate, six MFMAs per product; the transposed
// weights are split at pack time, layout.h "fragXT", the deltas in registers).  Reads what the fp32 / f32x3 training forwards saved (relu bits,
// raw outputs), writes what the weight-gradient kernels read (deltas[10][P][256] fp32, d_rgb[P][64], d_sig[P]) -- same buffers, same layouts.
// A delta row leaves for HBM while the NEXT (transposed) layer walks it as its B operand (the x3 core's row hook).
#include <hip/hip_runtime.h>
#include "kernels.h"
#include "launch.h"
#include "mlp_core_x3.h"
#include "mlp_train16.h"

namespace crnerf {

template <int NT>
__device__ __forceinline__ void zero_acc_x(f32x16 (&acc)[NT]) {
#pragma unroll
  for (int t = 0; t < NT; ++t)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[t][r] = 0.0f;
}

// delta = acc . relu' from the two mask words of this lane (word gg <-> g = h + 2 gg; bit 4T + r <-> feature 16T + 4g + r, i.e. register
// 4q + r of tile t with T = 2t + (q >> 1), gg = q & 1); MASK = false: the layer is linear
template <int NT, bool MASK>
__device__ __forceinline__ void finish_delta_x(const f32x16 (&acc)[NT], f32x16 (&dl)[8], unsigned long long m0, unsigned long long m1) {
#pragma unroll
  for (int t = 0; t < NT; ++t)
#pragma unroll
    for (int q = 0; q < 4; ++q)
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        float d = acc[t][4 * q + j];
        if (MASK) {
          const int bit = 4 * (2 * t + (q >> 1)) + j;
          const unsigned long long w = (q & 1) ? m1 : m0;
          d = ((w >> bit) & 1ull) ? d : 0.0f;
        }
        dl[t][4 * q + j] = d;
      }
}

__global__ __launch_bounds__(256, 1) void mlp_backward_x3_kernel(const char* __restrict__ packedT, const float* __restrict__ out, const float* __restrict__ d_out,
                                                                 const float* __restrict__ acts, float* __restrict__ deltas, float* __restrict__ d_rgb,
                                                                 float* __restrict__ d_sig, long P, int iters, const int* __restrict__ only_if) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  lds_char* lds = (lds_char*)smem;
  if (only_if && *only_if == 0) return;   // the h2 data gradient did the work (launch_mlp_backward)
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int p = lane & 31, h = lane >> 5;
  load_consts(lds, packedT, packedT);   // the consts block carries the sigma-head weights
  const lds_float* C = (const lds_float*)(lds + LDS_CONST0);
  WeightPipeX pipe;
  pipe.set_stream_frags(STREAMXT_FRAGS);
  pipe.start(lds, packedT + CONST_BYTES, packedT + CONST_BYTES, 1, 1, lane, wave);
  xu32x4 q[X_AHEAD];
  pipe.prime(q);
#pragma unroll 1
  for (int it = 0; it < iters; ++it) {
    const long tile = ((long)it * gridDim.x + blockIdx.x) * 4 + wave;
    const long n = tile * 32 + p;
    const bool valid = n < P;
    const long nn = valid ? n : 0;
    const float* orow = out + nn * OUT_DIM;
    const float* grow = d_out + nn * OUT_DIM;
    // the relu bits of this lane's features, all layers in one load batch per tile (words g = h and g = h + 2 of every slot but the linear one)
    unsigned long long b0[ACT_SLOTS], b1[ACT_SLOTS];
#pragma unroll
    for (int sl = 0; sl < ACT_SLOTS; ++sl) {
      b0[sl] = (valid && sl != 8) ? *mask_slot((float*)acts, P, sl, nn, h) : 0ull;
      b1[sl] = (valid && sl != 8) ? *mask_slot((float*)acts, P, sl, nn, h + 2) : 0ull;
    }
    const ActSaveX dsv{deltas, P, nn, valid, h};     // the x3 core's row saver, aimed at the delta rows
    const uint32_t vo = dsv.offset();

    f32x16 dl[8], acc[8];
    f32x16 drgb[2];                                   // static_rgb: sigmoid'            nerf.py:154,180
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
      for (int qq = 0; qq < 4; ++qq) {
        f32x4 v;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const float f = orow[32 * t + 8 * qq + 4 * h + j], gf = valid ? grow[32 * t + 8 * qq + 4 * h + j] : 0.0f;
          v[j] = gf * f * (1.0f - f);
          drgb[t][4 * qq + j] = v[j];
        }
        if (valid) *(f32x4*)(d_rgb + n * FEAT_DIM + 32 * t + 8 * qq + 4 * h) = v;
      }
    // static_sigma: softplus' = sigmoid(pre) = 1 - exp(-sigma)      nerf.py:146,172
    const float sg = orow[FEAT_DIM];
    const float dsp = valid ? grow[FEAT_DIM] * (1.0f - expf(-sg)) : 0.0f;
    if (valid && h == 0) d_sig[n] = dsp;

    {  // through static_rgb^T -> dir_encoding output (relu)
      f32x16 acc4[4];
      zero_acc_x<4>(acc4);
      mma_layer_x3<4, FEAT_DIM / 16, 0, 0>(pipe, drgb, drgb, acc4, q);
      finish_delta_x<4, true>(acc4, dl, b0[9], b1[9]);
    }
    zero_acc_x<8>(acc);                               // through dir_encoding^T[:, :256] -> xyz_encoding_final output (linear); delta_9 leaves on the way
    mma_layer_x3<8, 128 / 16, 0, 0, true, false>(pipe, dl, dl, acc, q, dsv.row(9), SaveRowX{}, vo);
    finish_delta_x<8, false>(acc, dl, 0ull, 0ull);
    zero_acc_x<8>(acc);                               // through xyz_encoding_final^T, + sigma head -> h8 (relu)
    mma_layer_x3<8, KS_HID, 0, 0, true, false>(pipe, dl, dl, acc, q, dsv.row(8), SaveRowX{}, vo);
#pragma unroll
    for (int t = 0; t < 8; ++t)
#pragma unroll
      for (int qq = 0; qq < 4; ++qq) {
        const f32x4 w = *(const __attribute__((address_space(3))) f32x4*)(C + C_WSIG + 32 * t + 8 * qq + 4 * h);
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[t][4 * qq + j] = fmaf(w[j], dsp, acc[t][4 * qq + j]);
      }
    finish_delta_x<8, true>(acc, dl, b0[7], b1[7]);
#pragma unroll 1
    for (int l = 7; l >= 1; --l) {                    // through xyz_encoding_{l+1}^T -> h_l (relu); l+1 = 8..2; delta_l leaves on the way
      zero_acc_x<8>(acc);
      mma_layer_x3<8, KS_HID, 0, 0, true, false>(pipe, dl, dl, acc, q, dsv.row(l), SaveRowX{}, vo);
      unsigned long long m0 = b0[0], m1 = b1[0];      // words of slot l - 1 by selects: a dynamic register index would go through M0, which the
#pragma unroll                                        // LDS-DMA asm (glds16) rewrites behind the compiler's back
      for (int t = 1; t < 7; ++t) { m0 = (l - 1 == t) ? b0[t] : m0; m1 = (l - 1 == t) ? b1[t] : m1; }
      finish_delta_x<8, true>(acc, dl, m0, m1);
    }
    {   // the first layer's deltas: nothing left to hide them behind
      const SaveRowX r0 = dsv.row(0);
#pragma unroll
      for (int t = 0; t < 8; ++t)
#pragma unroll
        for (int qq = 0; qq < 4; ++qq) {
          const xu32x4 v = {__float_as_uint(dl[t][4 * qq]), __float_as_uint(dl[t][4 * qq + 1]), __float_as_uint(dl[t][4 * qq + 2]), __float_as_uint(dl[t][4 * qq + 3])};
          __builtin_amdgcn_raw_buffer_store_b128(v, r0.rs, (int)(vo + 4u * (32 * t + 8 * qq)), 0, 0);
        }
    }
  }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
}

int launch_mlp_dgrad_x3(const void* packedT_x3, const float* out, const float* d_out, const float* acts, float* deltas, float* d_rgb, float* d_sig, long P,
                        hipStream_t stream, const int* only_if) {
  if (P <= 0) return 0;
  if ((unsigned long long)P * 1024ull >= (unsigned long long)SAVEX_OOB)
    return set_error(-2, "mlp_backward_x3: more than 3.9 M points per call (the delta rows are addressed with 32-bit offsets)");
  const GridPlan plan = plan_grid((P + 127) / 128);
  return launch_kernel(mlp_backward_x3_kernel, "mlp_backward_x3_kernel", plan.grid, 256, LDS_SCRATCH_X, stream, (const char*)packedT_x3, out, d_out, acts, deltas, d_rgb,
                       d_sig, P, plan.iters, only_if);
}

}  // namespace crnerf

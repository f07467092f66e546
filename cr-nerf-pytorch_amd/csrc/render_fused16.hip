// Fused volumetric renderer on the v16 core (mlp_core16.h): two wavefronts per SIMD.
// Contract: render_rays_cross_ray, models/rendering.py:50-196 (coarse pass, sample_pdf + merge, fine pass; outputs per A0 of SURVEY 8a).
//
// Work decomposition: workgroup = 8 waves = 4 rays; a ray belongs to a PAIR of waves (A = even wave,
// B = odd wave).  The ray's samples are walked in 32-sample steps; in step k wave A owns samples
// [32k, 32k+16), wave B [32k+16, 32k+32), each as one 16-point MFMA tile.  The pair exchanges only
// scalars through LDS: the product of (1-alpha) over each wave's 16 samples per step (running
// transmittance), and the per-ray feature/depth partial sums at the end of a pass.  sample_pdf and the
// merge run on the pair's 128 lanes.  All 8 waves execute identical control flow, so plain workgroup
// barriers order the exchanges.
#include <hip/hip_runtime.h>
#include "kernels.h"
#include "launch.h"
#include "mlp_core16.h"
#include "mlp_train16.h"
#include "pair_ops.h"
#include "ray_ops.h"

namespace crnerf {

struct RenderParams16 {
  const char* packed0; const char* packed1;
  const float* rays; const float* view_dir; const float* z_coarse; const float* z_steps; const float* u; long u_stride;
  const float* noise_c; const float* noise_f; float noise_std; int use_disp;
  long R; int Nc, Ni, iters;
  unsigned int* sched;   // null: static quad -> workgroup map (iters passes); else {next-quad counter, finished-workgroup counter}
  float* weights_c; float* feature_c; float* depth_c; float* weights_f; float* feature_f; float* depth_f; float* z_fine;
  // in-kernel random draws (include/crnerf.h, philox.h); rng_flags == 0: none
  unsigned long long rng_seed; long rng_ray_offset; int rng_flags; float perturb;
  float* z_coarse_out; float* noise_c_out; float* noise_f_out;
};

static __device__ unsigned int crnerf_sched16[SCHED_SLOTS][2];   // kernels.h "Dynamic work distribution"

// What the training twin adds to the renderer (crnerf_render_rays_train_f32): every tile's layer activations + relu bits
// (ActSaver, mlp_train16.h) and its raw MLP output row, per pass.  The inference kernel instantiates the no-op hook.
struct NoHook {
  static constexpr bool train = false;
  __device__ __forceinline__ NoSave saver(int, long, int, int, bool, int) const { return NoSave(); }
  __device__ __forceinline__ void raw(int, long, int, int, bool, int, const f32x4 (&)[4], float) const {}
};
struct TrainHook {
  static constexpr bool train = true;
  float* acts[2];   // [10][R*N][256] + masks, pass 0 = coarse (N = Nc), pass 1 = fine (N = Nc+Ni)
  float* rawo[2];   // [R*N][65]
  long R;
  __device__ __forceinline__ ActSaver saver(int pass, long r, int N, int n, bool ok, int g) const {
    return ActSaver{pass ? acts[1] : acts[0], R * N, r * N + n, ok, g};
  }
  __device__ __forceinline__ void raw(int pass, long r, int N, int n, bool ok, int g, const f32x4 (&feat)[4], float sigma) const {
    if (!ok) return;
    float* o = (pass ? rawo[1] : rawo[0]) + (r * N + n) * OUT_DIM;
#pragma unroll
    for (int T = 0; T < 4; ++T)
#pragma unroll
      for (int q = 0; q < 4; ++q) o[16 * T + 4 * g + q] = feat[T][q];
    if (g == 0) o[FEAT_DIM] = sigma;
  }
};

// RNG: the instantiation with the in-kernel random draws (philox.h).  It is a template parameter, not a runtime flag: the keys, the
// global ray index and three more output pointers would otherwise be live across the MLP of EVERY launch (measured: 10 -> 20
// spilled registers in the inference kernel, 77 -> 90 in the training twin).
// LEAN (crnerf_render_rays_lean_f32): the inference render that keeps only what an image needs.  The coarse pass exists for its compositing
// weights alone (they feed sample_pdf) and those depend on sigma alone, so its tiles walk the trunk only (WeightPipe16T<true>: 124 of the 151
// stages), no feature is composited and nothing of it is stored; the fine pass is the full one without the weights_fine store.  What is left
// executes the full kernel's instructions in the full kernel's order: feature_fine / depth_fine / z_fine are bit-identical.  A template
// parameter for the reason RNG is one: the other instantiations keep their code.
template <bool RNG, class HOOK, bool LEAN = false>
__device__ __forceinline__ void render_rays16_impl(const RenderParams16& a, const HOOK& hook) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  lds_char* lds = (lds_char*)smem;
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int p = lane & 15, g = lane >> 4;
  const int pair = wave >> 1, half = wave & 1;
  const int lane128 = half * 64 + lane;
  const int Nc = a.Nc, Ni = a.Ni, Nf = Nc + Ni;

  load_consts(lds, a.packed0, a.packed1);
  PairScratch scr;
  scr.bind(lds + LDS_SCRATCH + pair * PAIR_BYTES);
  lds_float* dirbuf = (lds_float*)(lds + LDS_SCRATCH + 4 * PAIR_BYTES) + wave * 32;   // 32 floats per wave

  const int steps_c = (Nc + 31) >> 5, steps_f = Ni > 0 ? (Nf + 31) >> 5 : 0;
  // the schedule levers (mlp_core16.h) are for the inference kernels; the training twins keep the unstaggered ring and compile to the code they had
  WeightPipe16T<LEAN, HOOK::train ? 0 : CRNERF_CORE16_LAG, !HOOK::train && CRNERF_CORE16_PRIO != 0> pipe;
  pipe.start(lds, a.packed0 + CONST_BYTES, a.packed1 + CONST_BYTES, steps_c, steps_c + steps_f, lane, wave);
  f32x4 q[V16_AHEAD];
  pipe.prime(q);
  PhaseTimer tm;
  tm.start(blockIdx.x == 0 && threadIdx.x == 0);

  // ray quads: statically strided over the grid, or (a.sched) pulled from a device counter -- the index for the NEXT pass is
  // requested at the top of a pass and picked up at its end, so the atomic's round trip is never waited for
  __attribute__((address_space(3))) unsigned int* qslot =
      (__attribute__((address_space(3))) unsigned int*)(lds + LDS_SCRATCH + 4 * PAIR_BYTES + V16_WAVES * 32 * sizeof(float));
  const long quads = (a.R + 3) / 4;
  long quad = blockIdx.x;
#pragma unroll 1
  for (int it = 0; a.sched ? quad < quads : it < a.iters; ++it) {
    unsigned int nxt = 0;
    if (a.sched && threadIdx.x == 0) nxt = gridDim.x + atomicAdd(a.sched, 1u);
    const long rr = quad * 4 + pair;
    const bool ray_ok = rr < a.R;
    const long r = ray_ok ? rr : a.R - 1;
    const float* ray = a.rays + r * 8;
    const float ox = ray[0], oy = ray[1], oz = ray[2], dx = ray[3], dy = ray[4], dz = ray[5];
    const float near = ray[6], far = ray[7];
    {
      const float* vd = a.view_dir ? a.view_dir + r * 3 : ray + 3;       // rendering.py:155
      f32x4 dv[2];
      posenc_regs16<DIR_FREQS, 2>(vd[0], vd[1], vd[2], g, dv);
      if (p == 0) {                                                      // per-ray constant: park it in LDS (DirLds)
        *(__attribute__((address_space(3))) f32x4*)(dirbuf + 8 * g) = dv[0];
        *(__attribute__((address_space(3))) f32x4*)(dirbuf + 8 * g + 4) = dv[1];
      }
    }
    const DirLds dirsrc{dirbuf + 8 * g};
    const RayRng rng{(uint32_t)(a.rng_seed & 0xffffffffu), (uint32_t)(a.rng_seed >> 32)};
    const long rng_ray = a.rng_ray_offset + r;
    for (int n = lane128; n < Nc; n += 128) {
      auto zlin = [&](int k) { return coarse_depth(near, far, a.z_steps ? a.z_steps[k] : linspace01(k, Nc), a.use_disp); };
      float zv;
      if (a.z_coarse) zv = a.z_coarse[r * Nc + n];
      else if (RNG && (a.rng_flags & 1)) {
        // rendering.py:169-176: mid-points, lower / upper interval ends, z = lower + (upper - lower) * (perturb * U[0,1))
        const float z0 = zlin(n);
        const float lower = n == 0 ? z0 : 0.5f * (zlin(n - 1) + z0);
        const float upper = n == Nc - 1 ? z0 : 0.5f * (z0 + zlin(n + 1));
        zv = lower + (upper - lower) * (a.perturb * rng.uniform(RNG_STREAM_JITTER, rng_ray, n));
      } else zv = zlin(n);
      scr.zc[n] = zv;
      if (RNG && a.z_coarse_out && ray_ok) a.z_coarse_out[r * Nc + n] = zv;
    }
    wg_barrier();

    const int npass = Ni > 0 ? 2 : 1;
#pragma unroll 1
    for (int pass = 0; pass < npass; ++pass) {
      const int N = pass ? Nf : Nc;
      const lds_float* zsrc = pass ? scr.zs : scr.zc;
      const float* noise_row = pass ? (a.noise_f ? a.noise_f + r * Nf : nullptr) : (a.noise_c ? a.noise_c + r * Nc : nullptr);
      float* weights_row = LEAN ? nullptr : (pass ? a.weights_f + r * Nf : a.weights_c + r * Nc);
      const bool compose = !LEAN || pass;     // wave-uniform, and the same in all eight waves
      double carry = 1.0;
      f32x4 facc[4];
#pragma unroll
      for (int T = 0; T < 4; ++T) facc[T] = f32x4{0, 0, 0, 0};
      float dacc = 0.0f;
      const int steps = (N + 31) >> 5;
#pragma unroll 1
      for (int k = 0; k < steps; ++k) {
        const int n = 32 * k + 16 * half + p;
        const bool valid = n < N;
        const int nc = valid ? n : N - 1;
        const float zn = zsrc[nc];
        const float znext = zsrc[nc + 1 < N ? nc + 1 : N - 1];
        const float x = ox + dx * zn, y = oy + dy * zn, z = oz + dz * zn;   // rendering.py:178 / :188
        f32x4 pe[6], feat[4];
        posenc_regs16<XYZ_FREQS, 6>(x, y, z, g, pe);
        float sigma;
        mlp_tile16(pipe, pass, pe, dirsrc, feat, sigma, g, q, tm, hook.saver(pass, r, N, n, valid && ray_ok, g));
        hook.raw(pass, r, N, n, valid && ray_ok, g, feat, sigma);
        // ---- compositing, rendering.py:121-143
        float noise = (noise_row && valid) ? noise_row[n] * a.noise_std : 0.0f;
        if (RNG && (a.rng_flags & 4) && valid) {          // rendering.py:125  noise = randn_like(sigma) * noise_std
          const float draw = rng.normal(pass ? RNG_STREAM_NOISE_FINE : RNG_STREAM_NOISE_COARSE, rng_ray, n);
          noise = draw * a.noise_std;
          float* no = pass ? a.noise_f_out : a.noise_c_out;
          if (no && ray_ok && g == 0) no[r * N + n] = draw;
        }
        const float delta = (n == N - 1) ? 1e2f : znext - zn;
        const float alpha = valid ? 1.0f - expf(-delta * fmaxf(sigma + noise, 0.0f)) : 0.0f;
        double incl = (double)(1.0f - alpha);
#pragma unroll
        for (int d = 1; d < 16; d <<= 1) {
          const double o = shfl_up_f64(incl, d, 16);
          if (p >= d) incl *= o;
        }
        double excl = shfl_up_f64(incl, 1, 16);
        if (p == 0) excl = 1.0;
        const double tot = shfl_f64(incl, 15, 16);
        if (lane == 0) scr.xprod[half] = tot;
        wg_barrier();
        const double other = scr.xprod[half ^ 1];
        const double prod_a = half ? other : tot, prod_b = half ? tot : other;
        const float Tr = (float)(half ? carry * prod_a * excl : carry * excl);
        carry = carry * prod_a * prod_b;
        const float w = alpha * Tr;
        if (compose) {
#pragma unroll
          for (int T = 0; T < 4; ++T)
#pragma unroll
            for (int rr2 = 0; rr2 < 4; ++rr2) facc[T][rr2] += w * feat[T][rr2];
          dacc += w * zn;
        }
        if (valid && g == 0) {
          if (!LEAN && ray_ok) weights_row[n] = w;
          if (pass == 0) scr.wc[n] = w;
        }
        tm.tick(T_COMPOSITE);
      }
      // per-wave reduction over the 16 point lanes, then pair combine through LDS (compose is tested per round: the form that spills least)
      {
#pragma unroll
        for (int d = 8; d >= 1; d >>= 1) if (compose) {
#pragma unroll
          for (int T = 0; T < 4; ++T)
#pragma unroll
            for (int rr2 = 0; rr2 < 4; ++rr2) facc[T][rr2] += __shfl_xor(facc[T][rr2], d);
          dacc += __shfl_xor(dacc, d);
        }
        if (compose && half == 1 && p == 0) {
#pragma unroll
          for (int T = 0; T < 4; ++T) *(__attribute__((address_space(3))) f32x4*)(scr.xfeat + 16 * T + 4 * g) = facc[T];
          if (g == 0) scr.xfeat[64] = dacc;
        }
      }
      wg_barrier();   // (a lean coarse pass too: the last step's scr.wc[] must be in LDS before sample_pdf_pair reads it)
      if (compose && half == 0 && p == 0 && ray_ok) {
        float* frow = (pass ? a.feature_f : a.feature_c) + r * FEAT_DIM;
#pragma unroll
        for (int T = 0; T < 4; ++T) {
          const f32x4 o = *(const __attribute__((address_space(3))) f32x4*)(scr.xfeat + 16 * T + 4 * g);
          *(f32x4*)(frow + 16 * T + 4 * g) = facc[T] + o;
        }
        if (g == 0) (pass ? a.depth_f : a.depth_c)[r] = dacc + scr.xfeat[64];
      }
      if (pass == 0 && Ni > 0) {
        sample_pdf_pair(scr, Nc, Ni, a.u ? a.u + r * a.u_stride : nullptr, lane, lane128, (RNG && (a.rng_flags & 2)) ? &rng : nullptr, rng_ray);
        wg_barrier();
        merge_sort_pair(scr, Nc, Ni, lane128);
        wg_barrier();
        if (a.z_fine && ray_ok)
          for (int n = lane128; n < Nf; n += 128) a.z_fine[r * Nf + n] = scr.zs[n];
      }
      tm.tick(T_RAYLEVEL);
    }
    if (a.sched && threadIdx.x == 0) *qslot = nxt;
    wg_barrier();   // scratch is rewritten by the next ray
    quad = a.sched ? (long)__builtin_amdgcn_readfirstlane((int)*qslot) : quad + gridDim.x;   // slot rewritten a whole pass later
  }
  if (a.sched && threadIdx.x == 0 && atomicAdd(a.sched + 1, 1u) == gridDim.x - 1) {   // last workgroup out: leave the slot zeroed
    atomicExch(a.sched, 0u);       // device-scope, like the increments: the per-XCD L2s are not coherent for plain stores
    atomicExch(a.sched + 1, 0u);
  }
  tm.flush();
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
}

__global__ __launch_bounds__(512, 2) void render_rays16_kernel(RenderParams16 a) { render_rays16_impl<false>(a, NoHook{}); }
__global__ __launch_bounds__(512, 2) void render_rays16_rng_kernel(RenderParams16 a) { render_rays16_impl<true>(a, NoHook{}); }
__global__ __launch_bounds__(512, 2) void render_rays16_lean_kernel(RenderParams16 a) { render_rays16_impl<false, NoHook, true>(a, NoHook{}); }

// Fused TRAINING forward: the same launch (posenc -> MLP -> compositing, coarse -> sample_pdf -> fine) that also keeps what
// the backward twins need -- no [P,93] / [P,120] embeddings and no separate compositing pass ever exist in HBM.
__global__ __launch_bounds__(512, 2) void render_rays_train16_kernel(RenderParams16 a, TrainHook h) { render_rays16_impl<false>(a, h); }
__global__ __launch_bounds__(512, 2) void render_rays_train16_rng_kernel(RenderParams16 a, TrainHook h) { render_rays16_impl<true>(a, h); }

int launch_render_rays16(const RenderArgs& a, hipStream_t stream) {
  if (a.R <= 0) return 0;
  if (int rc = check_sample_counts("render_rays", a, MAX_NC, MAX_NI)) return rc;
  RenderParams16 k;
  fill_render_params(k, a);
  fill_rng_params(k, a);
  const GridPlan plan = plan_grid((a.R + 3) / 4);
  k.iters = plan.iters;
  k.sched = k.iters > 1 ? sched_slot((const void*)crnerf_sched16) : nullptr;
  const size_t shmem = LDS_SCRATCH + 4 * PAIR_BYTES + V16_WAVES * 32 * sizeof(float) + 16;
  if (a.mode == RenderMode::Lean) {   // crnerf_render_rays_lean_f32: the coarse outputs and weights_fine are never written (abi.hip passes them as null)
    if (a.Ni < 1) return set_error(-2, "render_rays_lean: N_importance must be in [1, 256] (the coarse pass alone has nothing lean to return)");
    if (a.train_acts_coarse || a.rng_flags || a.z_coarse_out) return set_error(-3, "render_rays_lean: inference only, random draws come as tensors");
    return launch_kernel(render_rays16_lean_kernel, "render_rays16_lean_kernel", plan.grid, 512, shmem, stream, k);
  }
  const bool rngk = wants_rng_kernel(a);
  if (a.train_acts_coarse) {
    if (int rc = check_train_state("render_rays_train", a)) return rc;
    const TrainHook h{{(float*)a.train_acts_coarse, (float*)a.train_acts_fine}, {a.train_raw_coarse, a.train_raw_fine}, a.R};
    if (int rc = zero_train_ranges(a, stream)) return rc;     // the fp32 twin tracks no operand range (kernels.h)
    return launch_kernel(rngk ? render_rays_train16_rng_kernel : render_rays_train16_kernel, "render_rays_train16_kernel", plan.grid, 512, shmem, stream, k, h);
  }
  return launch_kernel(rngk ? render_rays16_rng_kernel : render_rays16_kernel, "render_rays16_kernel", plan.grid, 512, shmem, stream, k);
}

#ifdef CRNERF_TIMING
extern "C" int crnerf_debug_read_timing16(unsigned long long* host_out) {
  return (int)hipMemcpyFromSymbol(host_out, HIP_SYMBOL(crnerf_timing), sizeof(unsigned long long) * T_COUNT);
}
#endif

}  // namespace crnerf

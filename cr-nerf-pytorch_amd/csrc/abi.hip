// extern "C" surface of libcrnerf_hip.so -- see include/crnerf.h for the contract of every symbol.
#include <hip/hip_runtime.h>
#include <limits.h>
#include <mutex>
#include <stddef.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "../../include/crnerf.h"
#include "../../include/crnerf_blender.h"
#include "../../include/crnerf_geometry.h"
#include "../../include/crnerf_lean.h"
#include "../../include/crnerf_lean_x.h"
#include "../../include/crnerf_sweep.h"
#include "crnerf_point_features.h"
#include "crossray.h"
#include "kernels.h"
#include "layout.h"

namespace crnerf {

static thread_local char g_err[512] = "";

int set_error(int code, const char* msg) {
  snprintf(g_err, sizeof(g_err), "%s", msg);
  return code;
}

int check_launch(const char* what) {
  const hipError_t e = hipGetLastError();
  if (e == hipSuccess) return 0;
  snprintf(g_err, sizeof(g_err), "%s: %s", what, hipGetErrorString(e));
  return CRNERF_ERR_HIP;
}

int num_cus() {
  static int cached[64];
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) return 256;
  if (cached[dev] == 0) {
    int n = 0;
    if (hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || n <= 0) n = 256;
    cached[dev] = n;
  }
  return cached[dev];
}

// CU-share streams (include/crnerf.h).  The CU mask of hipExtStreamCreateWithCUMask is indexed in the driver's logical CU order, which on a
// multi-XCD part interleaves the XCDs (bit b = CU b / n_xcd of XCD b % n_xcd): a contiguous range of logical CUs of EVERY XCD is then the
// bit range [first * n_xcd, (first + count) * n_xcd).  n_xcd = 8 on gfx950 (256 CUs = 8 x 32).
static const int N_XCD = 8;
extern "C" int crnerf_cus_per_xcd(void) { return num_cus() / N_XCD; }
extern "C" int crnerf_stream_create_cu_share(void** stream, int first, int count) {
  if (!stream) return set_error(-1, "stream_create_cu_share: stream is NULL");
  const int per = num_cus() / N_XCD;
  if (first < 0 || count <= 0 || first + count > per) return set_error(-3, "stream_create_cu_share: [first, first + count) must lie inside crnerf_cus_per_xcd()");
  uint32_t mask[16] = {0};
  for (int b = first * N_XCD; b < (first + count) * N_XCD; ++b) mask[b >> 5] |= 1u << (b & 31);
  hipStream_t st = nullptr;
  const hipError_t e = hipExtStreamCreateWithCUMask(&st, (uint32_t)((num_cus() + 31) / 32), mask);
  if (e != hipSuccess) {
    static thread_local char msg[160];
    snprintf(msg, sizeof msg, "stream_create_cu_share: hipExtStreamCreateWithCUMask: %s", hipGetErrorString(e));
    return set_error(-1, msg);
  }
  *stream = (void*)st;
  return 0;
}
extern "C" int crnerf_stream_destroy(void* stream) {
  if (!stream) return 0;
  return hipStreamDestroy((hipStream_t)stream) == hipSuccess ? 0 : set_error(-1, "stream_destroy: hipStreamDestroy failed");
}

unsigned int* sched_slot(const void* symbol) {
  static std::mutex mu;
  static int cursor = 0;
  void* base = nullptr;
  if (hipGetSymbolAddress(&base, symbol) != hipSuccess || !base) return nullptr;
  std::lock_guard<std::mutex> lock(mu);
  const int k = cursor++ % SCHED_SLOTS;
  return (unsigned int*)base + 2 * k;
}

int ensure_dynamic_lds(const void* fn, size_t bytes, const char* what) {
  struct Slot { const void* fn; int dev; size_t bytes; };
  static Slot slots[128];
  static int n_slots = 0;
  static std::mutex mu;
  int dev = 0;
  (void)hipGetDevice(&dev);
  std::lock_guard<std::mutex> lock(mu);
  Slot* s = nullptr;
  for (int i = 0; i < n_slots; ++i)
    if (slots[i].fn == fn && slots[i].dev == dev) { s = &slots[i]; break; }
  if (s && s->bytes >= bytes) return 0;
  if (hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes) != hipSuccess) {
    char msg[160];
    snprintf(msg, sizeof(msg), "hipFuncSetAttribute(%s, %zu bytes of LDS) failed", what, bytes);
    return set_error(-10, msg);
  }
  if (!s && n_slots < 128) s = &slots[n_slots++];
  if (s) { s->fn = fn; s->dev = dev; s->bytes = bytes; }
  return 0;
}

}  // namespace crnerf

using namespace crnerf;

#define REQUIRE(p, name) \
  if (!(p)) return set_error(CRNERF_ERR_NULL, name " is NULL")

// "<who>: <what>" -- composed here, on the failure path only, for the rules that several entry points share
static int fail(int code, const char* who, const char* what) {
  static thread_local char msg[160];
  snprintf(msg, sizeof msg, "%s: %s", who, what);
  return set_error(code, msg);
}

// every entry of a host list of n pointers (of two such lists) is set
template <class A>
static bool all_set(A* const* list, int n) {
  for (int i = 0; i < n; ++i)
    if (!list[i]) return false;
  return true;
}
template <class A, class B>
static bool all_set2(A* const* a, B* const* b, int n) { return all_set(a, n) && all_set(b, n); }

static MlpTensors to_tensors(const float* const* tensors) {
  MlpTensors t;
  for (int i = 0; i < 8; ++i) { t.w[i] = tensors[2 * i]; t.b[i] = tensors[2 * i + 1]; }
  t.w_final = tensors[16]; t.b_final = tensors[17];
  t.w_sigma = tensors[18]; t.b_sigma = tensors[19];
  t.w_dir = tensors[20]; t.b_dir = tensors[21];
  t.w_rgb = tensors[22]; t.b_rgb = tensors[23];
  return t;
}

static int null_tensor(const char* who) { return fail(CRNERF_ERR_NULL, who, "a tensor pointer is NULL"); }

// the 24 tensors of a NeRF_sigma are all set
static int require_tensors(const char* who, const float* const* tensors) { return all_set(tensors, CRNERF_MLP_TENSORS) ? 0 : null_tensor(who); }

// every crnerf_pack_mlp_weights*: launch(MlpTensors, packed, hipStream_t) is the layout's packer
template <class Launch>
static int pack_entry(const char* who, const float* const* tensors, void* packed, void* stream, Launch launch) {
  REQUIRE(tensors, "tensors"); REQUIRE(packed, "packed");
  if (int rc = require_tensors(who, tensors)) return rc;
  return launch(to_tensors(tensors), packed, (hipStream_t)stream);
}

// every crnerf_mlp_forward_*: launch(P) runs the core on the P = n points
template <class Launch>
static int forward_entry(const char* who, const void* packed, const float* x, float* out, int64_t n, Launch launch) {
  if (n == 0) return 0;
  REQUIRE(packed, "packed"); REQUIRE(x, "x"); REQUIRE(out, "out");
  if (n < 0) return fail(CRNERF_ERR_SHAPE, who, "negative n");
  return launch((long)n);
}

// every crnerf_sigma_points_* / crnerf_sigma_grid_* (include/crnerf_geometry.h): the kernels index points with 32 bits
static const int64_t SIGMA_MAX_POINTS = 0x7fffffffLL;
template <class Launch>
static int sigma_points_entry(const void* packed, const float* xyz, float* sigma, int64_t n, Launch launch) {
  if (n < 0) return fail(CRNERF_ERR_SHAPE, "sigma_points", "negative n");
  if (n == 0) return 0;
  REQUIRE(packed, "packed"); REQUIRE(xyz, "xyz"); REQUIRE(sigma, "sigma");
  if (n > SIGMA_MAX_POINTS) return fail(CRNERF_ERR_SHAPE, "sigma_points", "more than 2^31 - 1 points in one call (split the list)");
  return launch((long)n);
}
// every crnerf_feature_points_* (crnerf_point_features.h): the density query's rules, with a direction per point; sigma may be NULL
template <class Launch>
static int feature_points_entry(const void* packed, const float* xyz, const float* dirs, float* feature, int64_t n, Launch launch) {
  if (n < 0) return fail(CRNERF_ERR_SHAPE, "feature_points", "negative n");
  if (n == 0) return 0;
  REQUIRE(packed, "packed"); REQUIRE(xyz, "xyz"); REQUIRE(dirs, "dirs"); REQUIRE(feature, "feature");
  if (n > SIGMA_MAX_POINTS) return fail(CRNERF_ERR_SHAPE, "feature_points", "more than 2^31 - 1 points in one call (split the list)");
  return launch((long)n);
}
template <class Launch>
static int sigma_grid_entry(const void* packed, const float* xs, const float* ys, const float* zs, int32_t nx, int32_t ny, int32_t nz, float* sigma,
                            Launch launch) {
  if (nx < 0 || ny < 0 || nz < 0) return fail(CRNERF_ERR_SHAPE, "sigma_grid", "negative axis length");
  if (nx == 0 || ny == 0 || nz == 0) return 0;
  REQUIRE(packed, "packed"); REQUIRE(xs, "xs"); REQUIRE(ys, "ys"); REQUIRE(zs, "zs"); REQUIRE(sigma, "sigma");
  // (nx * ny < 2^62, and the quotient test keeps the triple product out of 64-bit overflow)
  if ((int64_t)nx * ny > SIGMA_MAX_POINTS / nz) return fail(CRNERF_ERR_SHAPE, "sigma_grid", "more than 2^31 - 1 points in one call (slabs of a grid are grids)");
  return launch();
}

// the 22 decoder tensors in kernel order (CRNERF_DECODER_TENSORS); a backward entry leaves workspace, rgb and plane_stride null
static DecodeArgs to_decode_args(const float* content, int64_t HW, const float* style, int64_t HWs, const float* const* w, void* workspace = nullptr,
                                 float* rgb = nullptr, int64_t plane_stride = 0) {
  DecodeArgs d;
  d.content = content; d.HW = (long)HW; d.style = style; d.HWs = (long)HWs;
  d.snet = CnnTensors{w[0], w[1], w[2], w[3], w[4], w[5]}; d.snet_fc_w = w[6]; d.snet_fc_b = w[7];
  d.cnet = CnnTensors{w[8], w[9], w[10], w[11], w[12], w[13]}; d.cnet_fc_w = w[14]; d.cnet_fc_b = w[15];
  d.lin = FoldTensors{w[16], w[17], w[18], w[19], w[20], w[21]};
  d.workspace = workspace; d.rgb = rgb; d.plane_stride = (long)plane_stride;
  return d;
}

// The single place that fills a RenderArgs from the ABI's struct; an entry point's own differences are overrides behind it.  The rng fields stay
// at their defaults (perturb == 0) unless rng_flags asks for in-kernel draws, whatever the caller left in the struct.
static RenderArgs to_render_args(const crnerf_render_args* a) {
  RenderArgs r;
  r.packed_coarse = a->packed_coarse; r.packed_fine = a->packed_fine; r.rays = a->rays; r.view_dir = a->view_dir;
  r.z_coarse = a->z_coarse; r.z_steps = a->z_steps; r.u = a->u; r.u_stride = (long)a->u_stride; r.noise_coarse = a->noise_coarse; r.noise_fine = a->noise_fine;
  r.noise_std = a->noise_std; r.use_disp = a->use_disp; r.R = (long)a->n_rays; r.Nc = a->n_samples; r.Ni = a->n_importance;
  r.weights_coarse = a->weights_coarse; r.feature_coarse = a->feature_coarse; r.depth_coarse = a->depth_coarse;
  r.weights_fine = a->weights_fine; r.feature_fine = a->feature_fine; r.depth_fine = a->depth_fine; r.z_fine = a->z_fine;
  if (a->rng_flags) { r.rng_seed = a->rng_seed; r.rng_ray_offset = (long)a->rng_ray_offset; r.rng_flags = a->rng_flags; r.perturb = a->perturb; }
  r.z_coarse_out = a->z_coarse_out; r.noise_coarse_out = a->noise_coarse_out; r.noise_fine_out = a->noise_fine_out;
  return r;
}

// the kernel family behind a crnerf_render_rays_* entry
enum class Core {
  F32,         // inference and the fp32 training twin
  BF16_PAIR,   // the pair core: inference and the mixed-precision training twin
  F16_PAIR,    // its fp16-operand build; inference only
  X3,          // three bf16 pieces
  H2,          // two fp16 pieces
  X3_REPAIR,   // the x3 core on the ray quads that hold a NaN
};
// the pair cores draw nothing in the kernel and write no *_out
static bool is_pair_core(Core c) { return c == Core::BF16_PAIR || c == Core::F16_PAIR; }

// what a training twin saves per pass; all null: inference
struct TrainState { void* acts_coarse = nullptr; void* acts_fine = nullptr; float* raw_coarse = nullptr; float* raw_fine = nullptr; };

static int require_train_state(const crnerf_render_args* a, const TrainState& t) {
  REQUIRE(t.acts_coarse, "acts_coarse"); REQUIRE(t.raw_coarse, "raw_coarse");
  if (a->n_importance > 0) { REQUIRE(t.acts_fine, "acts_fine"); REQUIRE(t.raw_fine, "raw_fine"); REQUIRE(a->z_fine, "z_fine"); }
  return 0;
}

// A pointer field of crnerf_render_args: where it is, and what is said when it is missing
struct Field { size_t at; const char* null_text; };
typedef crnerf_render_args A;
static const Field PACKED_COARSE = {offsetof(A, packed_coarse), "packed_coarse is NULL"}, PACKED_FINE = {offsetof(A, packed_fine), "packed_fine is NULL"}, RAYS = {offsetof(A, rays), "rays is NULL"},
                   U = {offsetof(A, u), "u is NULL"}, NOISE_COARSE = {offsetof(A, noise_coarse), "noise_coarse is NULL"}, NOISE_FINE = {offsetof(A, noise_fine), "noise_fine is NULL"},
                   WEIGHTS_COARSE = {offsetof(A, weights_coarse), "weights_coarse is NULL"}, WEIGHTS_COARSE_IN = {offsetof(A, weights_coarse), "weights_coarse (input) is NULL"},
                   FEATURE_COARSE = {offsetof(A, feature_coarse), "feature_coarse is NULL"}, DEPTH_COARSE = {offsetof(A, depth_coarse), "depth_coarse is NULL"},
                   WEIGHTS_FINE = {offsetof(A, weights_fine), "weights_fine is NULL"}, FEATURE_FINE = {offsetof(A, feature_fine), "feature_fine is NULL"},
                   DEPTH_FINE = {offsetof(A, depth_fine), "depth_fine is NULL"}, Z_FINE = {offsetof(A, z_fine), "z_fine is NULL"};

// the range an entry accepts a sample count in; what == nullptr: no rule of the entry's own (the launch layer's stand)
struct Range { int lo, hi, code; const char* what; };
static const Range LEAN_NI = {1, 256, CRNERF_ERR_SHAPE, "n_importance must be in [1, 256]"}, LEAN_NS = {3, 256, CRNERF_ERR_SHAPE, "n_samples must be in [3, 256]"};

// One render entry: what it checks, in the order render_entry checks it, and what it hands its launcher.  The Field lists end at an empty Field.
struct RenderEntry {
  const char* who;                // the name in its error texts
  Range n_importance, n_samples;
  Field required[7];              // non-null, asked for in this order
  Field required_fine[5];         // the same, when n_importance > 0
  const char* no_draws;           // the one refusal of rng_flags and the three *_out; nullptr: render_rays' rule by rule (check_draws)
  RenderMode mode;
  Field ignored[10];              // null for the launcher, whatever the caller passed
};
static const RenderEntry
    RENDER_RAYS = {"render_rays", {}, {}, {PACKED_COARSE, RAYS, WEIGHTS_COARSE, FEATURE_COARSE, DEPTH_COARSE}, {PACKED_FINE, WEIGHTS_FINE, FEATURE_FINE, DEPTH_FINE},
                   nullptr, RenderMode::Full, {}},
    // no coarse pass: one pack, the fine model's, and weights_coarse is the INPUT
    BF16_FINE = {"render_rays_bf16_fine", {1, INT_MAX, CRNERF_ERR_CONFIG, "n_importance must be > 0"}, {},
                 {PACKED_FINE, RAYS, WEIGHTS_COARSE_IN, WEIGHTS_FINE, FEATURE_FINE, DEPTH_FINE}, {},
                 "no in-kernel random draws in the bf16 kernels", RenderMode::FineOnly, {NOISE_COARSE, FEATURE_COARSE, DEPTH_COARSE}},
    LEAN = {"render_rays_lean", LEAN_NI, LEAN_NS, {PACKED_COARSE, PACKED_FINE, RAYS, FEATURE_FINE, DEPTH_FINE}, {},
            "no in-kernel random draws in the lean kernel (hand them over as z_coarse / u / noise_*)", RenderMode::Lean,
            {WEIGHTS_COARSE, FEATURE_COARSE, DEPTH_COARSE, WEIGHTS_FINE}},
    // include/crnerf_lean_composite.h: the coarse pass for its compositing weights alone, and the lean fine launch behind it
    COARSE_WEIGHTS = {"render_coarse_weights", {0, 0, CRNERF_ERR_SHAPE, "n_importance must be 0 (the fine pass is crnerf_render_rays_lean_bf16_fine)"},
                      {2, 256, CRNERF_ERR_SHAPE, "n_samples must be in [2, 256]"}, {PACKED_COARSE, RAYS, WEIGHTS_COARSE}, {},
                      "no in-kernel random draws (hand them over as z_coarse / noise_coarse)", RenderMode::CoarseWeights,
                      {PACKED_FINE, U, NOISE_FINE, FEATURE_COARSE, DEPTH_COARSE, WEIGHTS_FINE, FEATURE_FINE, DEPTH_FINE, Z_FINE}},
    LEAN_BF16_FINE = {"render_rays_lean_bf16_fine", LEAN_NI, LEAN_NS, {PACKED_FINE, RAYS, WEIGHTS_COARSE_IN, FEATURE_FINE, DEPTH_FINE}, {},
                      "no in-kernel random draws in the bf16 kernels", RenderMode::LeanFineOnly, {NOISE_COARSE, FEATURE_COARSE, DEPTH_COARSE, WEIGHTS_FINE}};

static int require_fields(const crnerf_render_args* a, const Field* list) {
  for (const void* p; list->null_text; ++list) {
    memcpy(&p, (const char*)a + list->at, sizeof p);
    if (!p) return set_error(CRNERF_ERR_NULL, list->null_text);
  }
  return 0;
}
static int check_range(const RenderEntry& e, const Range& r, int n) { return (r.what && (n < r.lo || n > r.hi)) ? fail(r.code, e.who, r.what) : 0; }

// crnerf_render_rays_*: what may be drawn in the kernel, flag by flag
static int check_draws(const crnerf_render_args* a, Core core) {
  if (a->rng_flags) {
    if (a->rng_flags & ~(CRNERF_RNG_JITTER | CRNERF_RNG_U | CRNERF_RNG_NOISE)) return set_error(CRNERF_ERR_CONFIG, "render_rays: unknown rng_flags bits");
    if (is_pair_core(core)) return set_error(CRNERF_ERR_CONFIG, "render_rays: in-kernel random draws exist in the fp32, f32x3 and f32h2 kernels only");
    if ((a->rng_flags & CRNERF_RNG_JITTER) && a->z_coarse) return set_error(CRNERF_ERR_CONFIG, "render_rays: CRNERF_RNG_JITTER and z_coarse are exclusive");
    if ((a->rng_flags & CRNERF_RNG_U) && a->u) return set_error(CRNERF_ERR_CONFIG, "render_rays: CRNERF_RNG_U and u are exclusive");
    if ((a->rng_flags & CRNERF_RNG_NOISE) && (a->noise_coarse || a->noise_fine)) return set_error(CRNERF_ERR_CONFIG, "render_rays: CRNERF_RNG_NOISE and noise_* are exclusive");
  }
  if ((a->z_coarse_out || a->noise_coarse_out || a->noise_fine_out) && is_pair_core(core))   // (the bf16 kernels do not write them)
    return set_error(CRNERF_ERR_CONFIG, "render_rays: z_coarse_out / noise_*_out are written by the fp32, f32x3 and f32h2 kernels only");
  return 0;
}

static int launch_core(Core core, RenderArgs& r, hipStream_t stream) {
  switch (core) {
    case Core::H2: return launch_render_rays_h2(r, stream);
    case Core::X3_REPAIR: r.repair = 1; [[fallthrough]];
    case Core::X3: return launch_render_rays_x3(r, stream);
    case Core::F16_PAIR: return launch_render_rays_f16p(r, stream);
    case Core::BF16_PAIR: return launch_render_rays_bf16p(r, stream);
    case Core::F32: break;
  }
  return launch_render_rays16(r, stream);
}

// The sequence every render entry follows.
static int render_entry(const crnerf_render_args* a, void* stream, const RenderEntry& e, Core core, const TrainState& train = TrainState()) {
  REQUIRE(a, "args");
  if (a->n_rays == 0) return 0;
  if (a->n_rays < 0) return fail(CRNERF_ERR_SHAPE, e.who, "negative n_rays");
  if (int rc = check_range(e, e.n_importance, a->n_importance)) return rc;
  if (int rc = check_range(e, e.n_samples, a->n_samples)) return rc;
  if (int rc = require_fields(a, e.required)) return rc;
  if (a->n_importance > 0)
    if (int rc = require_fields(a, e.required_fine)) return rc;
  if (!e.no_draws) {
    if (int rc = check_draws(a, core)) return rc;
  } else if (a->rng_flags || a->z_coarse_out || a->noise_coarse_out || a->noise_fine_out) {
    return fail(CRNERF_ERR_CONFIG, e.who, e.no_draws);
  }
  crnerf_render_args b = *a;
  for (const Field* f = e.ignored; f->null_text; ++f) memset((char*)&b + f->at, 0, sizeof(void*));
  if (e.mode == RenderMode::FineOnly || e.mode == RenderMode::LeanFineOnly) b.packed_coarse = b.packed_fine;
  auto r = to_render_args(&b);
  r.mode = e.mode;
  r.train_acts_coarse = train.acts_coarse; r.train_acts_fine = train.acts_fine; r.train_raw_coarse = train.raw_coarse; r.train_raw_fine = train.raw_fine;
  return launch_core(core, r, (hipStream_t)stream);
}

// the five crnerf_render_rays_train_*: the saved state is checked before anything render_entry checks
static int render_rays_train(const crnerf_render_args* a, const TrainState& train, void* stream, Core core) {
  REQUIRE(a, "args");
  if (a->n_rays == 0) return 0;
  if (int rc = require_train_state(a, train)) return rc;
  return render_entry(a, stream, RENDER_RAYS, core, train);
}

extern "C" {

int crnerf_abi_version(void) { return CRNERF_ABI_VERSION; }
const char* crnerf_last_error(void) { return g_err; }
size_t crnerf_packed_mlp_bytes(void) { return PACKED_BYTES; }
size_t crnerf_crossray_workspace_bytes(void) { return CROSSRAY_WORKSPACE_BYTES; }

int crnerf_pack_mlp_weights(const float* const* tensors, void* packed, void* stream) {
  return pack_entry("pack_mlp_weights", tensors, packed, stream, launch_pack_mlp);
}

size_t crnerf_packed_mlp_t_bytes(void) { return PACKEDT_BYTES; }
size_t crnerf_mlp_train_acts_bytes(int64_t n) { return mlp_train_acts_bytes((long)n); }
size_t crnerf_mlp_train_scratch_bytes(int64_t n) { return mlp_train_scratch_bytes((long)n); }

int crnerf_pack_mlp_weights_t(const float* const* tensors, void* packed_t, void* stream) {
  REQUIRE(tensors, "tensors"); REQUIRE(packed_t, "packed_t");     // (this entry's message names the pack "packed_t")
  return pack_entry("pack_mlp_weights_t", tensors, packed_t, stream, launch_pack_mlpT);
}

int crnerf_mlp_forward_train_f32(const void* packed, const float* x, float* out, void* acts, int64_t n, void* stream) {
  if (n == 0) return 0;
  REQUIRE(packed, "packed"); REQUIRE(x, "x"); REQUIRE(out, "out"); REQUIRE(acts, "acts");
  return launch_mlp_forward_train(packed, x, out, (float*)acts, (long)n, (hipStream_t)stream);
}

// Flag and pointer checks shared by the three crnerf_mlp_backward_*_f32 entries.  `modes`: the weight-gradient modes this entry accepts (exclusive);
// CRNERF_BWD_PHASE_DGRAD / _WGRAD choose which half runs and with it which pointers are read.
static int check_backward_args(const char* who, int flags, int modes, const void* packed_t, const float* x, const float* out, const float* d_out,
                               const void* acts, const void* scratch, float* const* grads) {
  const int phases = CRNERF_BWD_PHASE_DGRAD | CRNERF_BWD_PHASE_WGRAD;
  if (flags & ~(modes | phases)) return fail(CRNERF_ERR_CONFIG, who, "unknown flag bits");
  const int m = flags & modes;
  if ((m & (m - 1)) != 0) return fail(CRNERF_ERR_CONFIG, who, "the weight-gradient modes are exclusive");
  const bool dgrad = (flags & phases) != CRNERF_BWD_PHASE_WGRAD, wgrad = (flags & phases) != CRNERF_BWD_PHASE_DGRAD;
  const char* missing = !acts ? "acts" : !scratch ? "scratch" : (dgrad && !packed_t) ? "packed_t" : (dgrad && !out) ? "out" : (dgrad && !d_out) ? "d_out" :
                        (wgrad && !x) ? "x" : (wgrad && !grads) ? "grads" : nullptr;
  if (missing) {
    static thread_local char msg[160];
    snprintf(msg, sizeof msg, "%s: %s is NULL", who, missing);
    return set_error(CRNERF_ERR_NULL, msg);
  }
  if (wgrad && !all_set(grads, CRNERF_MLP_TENSORS)) return fail(CRNERF_ERR_NULL, who, "a gradient pointer is NULL");
  return 0;
}

int crnerf_mlp_backward_f32(const void* packed_t, const float* x, const float* out, const float* d_out, const void* acts, void* scratch,
                            float* const* grads, int64_t n, void* stream) {
  return crnerf_mlp_backward_ex_f32(packed_t, x, out, d_out, acts, scratch, grads, n, 0, stream);
}

int crnerf_mlp_backward_ex_f32(const void* packed_t, const float* x, const float* out, const float* d_out, const void* acts, void* scratch,
                               float* const* grads, int64_t n, int flags, void* stream) {
  if (n == 0) return 0;
  if (int rc = check_backward_args("mlp_backward_ex", flags, CRNERF_BWD_WGRAD_BF16 | CRNERF_BWD_WGRAD_BF16X3, packed_t, x, out, d_out, acts, scratch, grads)) return rc;
  return launch_mlp_backward(packed_t, x, out, d_out, (const float*)acts, scratch, grads, (long)n, (hipStream_t)stream, flags);
}

int crnerf_posenc_f32(const float* x, float* out, int64_t n, int n_freqs, void* stream) {
  if (n == 0) return 0;
  REQUIRE(x, "x");
  REQUIRE(out, "out");
  if (n < 0) return set_error(CRNERF_ERR_SHAPE, "posenc: negative n");
  return launch_posenc(x, out, (long)n, n_freqs, (hipStream_t)stream);
}

int crnerf_embed_points_f32(const float* rays, const float* z, const float* dir_emb, float* x, int64_t n_rays, int32_t n_samples, void* stream) {
  if (n_rays == 0 || n_samples == 0) return 0;
  REQUIRE(rays, "rays"); REQUIRE(z, "z"); REQUIRE(dir_emb, "dir_emb"); REQUIRE(x, "x");
  if (n_rays < 0 || n_samples < 0) return set_error(CRNERF_ERR_SHAPE, "embed_points: negative size");
  return launch_embed_points(rays, z, dir_emb, x, (long)n_rays, (int)n_samples, (hipStream_t)stream);
}

int crnerf_mlp_forward_f32(const void* packed, const float* x, float* out, int64_t n, int sigma_only, void* stream) {
  return forward_entry("mlp_forward", packed, x, out, n, [&](long P) { return launch_mlp_forward16(packed, x, out, P, sigma_only, (hipStream_t)stream); });
}

int crnerf_composite_f32(const float* raw, const float* z, const float* noise, float noise_std, float* weights, float* feature,
                         float* depth, int64_t R, int N, void* stream) {
  if (R == 0) return 0;
  REQUIRE(raw, "raw"); REQUIRE(z, "z"); REQUIRE(weights, "weights"); REQUIRE(feature, "feature"); REQUIRE(depth, "depth");
  if (R < 0) return set_error(CRNERF_ERR_SHAPE, "composite: negative R");
  return launch_composite(raw, z, noise, noise_std, weights, feature, depth, (long)R, N, (hipStream_t)stream);
}

int crnerf_composite_backward_f32(const float* raw, const float* z, const float* noise, float noise_std, const float* d_feature,
                                  const float* d_depth, const float* d_weights, float* d_raw, int64_t R, int N, void* stream) {
  if (R == 0) return 0;
  REQUIRE(raw, "raw"); REQUIRE(z, "z"); REQUIRE(d_feature, "d_feature"); REQUIRE(d_raw, "d_raw");
  if (R < 0) return set_error(CRNERF_ERR_SHAPE, "composite_backward: negative R");
  return launch_composite_backward(raw, z, noise, noise_std, d_feature, d_depth, d_weights, d_raw, (long)R, N, (hipStream_t)stream);
}

int crnerf_sample_pdf_merge_f32(const float* z_coarse, const float* weights_coarse, const float* u, int64_t u_stride, float* z_sorted,
                                float* z_samples, int64_t R, int Nc, int Ni, void* stream) {
  if (R == 0) return 0;
  REQUIRE(z_coarse, "z_coarse"); REQUIRE(weights_coarse, "weights_coarse"); REQUIRE(z_sorted, "z_sorted");
  if (R < 0) return set_error(CRNERF_ERR_SHAPE, "sample_pdf_merge: negative R");
  return launch_sample_pdf_merge(z_coarse, weights_coarse, u, (long)u_stride, z_sorted, z_samples, (long)R, Nc, Ni, (hipStream_t)stream);
}

int crnerf_render_rays_f32(const crnerf_render_args* a, void* stream) { return render_entry(a, stream, RENDER_RAYS, Core::F32); }
int crnerf_rng_fill_f32(float* out, int64_t n_rays, int n, uint64_t seed, int stream_id, int64_t ray_offset, void* stream) {
  if (n_rays == 0 || n == 0) return 0;
  REQUIRE(out, "out");
  if (n_rays < 0 || n < 0) return set_error(CRNERF_ERR_SHAPE, "rng_fill: negative size");
  if (stream_id < 0 || stream_id > 3) return set_error(CRNERF_ERR_CONFIG, "rng_fill: stream must be 0..3");
  return launch_rng_fill(out, (long)n_rays, n, seed, stream_id, (long)ray_offset, (hipStream_t)stream);
}

int crnerf_render_rays_bf16(const crnerf_render_args* a, void* stream) { return render_entry(a, stream, RENDER_RAYS, Core::BF16_PAIR); }

int crnerf_render_rays_bf16_fine(const crnerf_render_args* a, void* stream) { return render_entry(a, stream, BF16_FINE, Core::BF16_PAIR); }
int crnerf_render_rays_lean_f32(const crnerf_render_args* a, void* stream) { return render_entry(a, stream, LEAN, Core::F32); }
// include/crnerf_lean.h
int crnerf_render_rays_lean_bf16(const crnerf_render_args* a, void* stream) { return render_entry(a, stream, LEAN, Core::BF16_PAIR); }
int crnerf_render_rays_lean_f16(const crnerf_render_args* a, void* stream) { return render_entry(a, stream, LEAN, Core::F16_PAIR); }
// include/crnerf_lean_composite.h
int crnerf_render_coarse_weights_f32h2(const crnerf_render_args* a, void* stream) { return render_entry(a, stream, COARSE_WEIGHTS, Core::H2); }
int crnerf_render_coarse_weights_f32x3(const crnerf_render_args* a, void* stream) { return render_entry(a, stream, COARSE_WEIGHTS, Core::X3); }
int crnerf_render_coarse_weights_f32x3_repair(const crnerf_render_args* a, void* stream) { return render_entry(a, stream, COARSE_WEIGHTS, Core::X3_REPAIR); }
int crnerf_render_coarse_weights_f16(const crnerf_render_args* a, void* stream) { return render_entry(a, stream, COARSE_WEIGHTS, Core::F16_PAIR); }
int crnerf_render_rays_lean_bf16_fine(const crnerf_render_args* a, void* stream) { return render_entry(a, stream, LEAN_BF16_FINE, Core::BF16_PAIR); }
// include/crnerf_lean_x.h
int crnerf_render_rays_lean_f32x3(const crnerf_render_args* a, void* stream) { return render_entry(a, stream, LEAN, Core::X3); }
int crnerf_render_rays_lean_f32h2(const crnerf_render_args* a, void* stream) { return render_entry(a, stream, LEAN, Core::H2); }
int crnerf_render_rays_lean_f32x3_repair(const crnerf_render_args* a, void* stream) { return render_entry(a, stream, LEAN, Core::X3_REPAIR); }

size_t crnerf_packed_mlp_mixed_bytes(void) { return gemm_packed_bytes(); }
size_t crnerf_mlp_train_mixed_acts_bytes(int64_t n) { return mlp_train_mixed_acts_bytes((long)n); }
size_t crnerf_mlp_train_mixed_scratch_bytes(int64_t n) { return mlp_train_mixed_scratch_bytes((long)n); }

int crnerf_pack_mlp_weights_mixed(const float* const* tensors, void* packed, void* stream) {
  return pack_entry("pack_mlp_weights_mixed", tensors, packed, stream, launch_pack_mlp_gemm);
}

int crnerf_mlp_forward_train_mixed_f32(const float* const* tensors, const void* packed, const float* x, float* out, void* acts, int64_t n,
                                       void* stream) {
  if (n == 0) return 0;
  REQUIRE(tensors, "tensors"); REQUIRE(packed, "packed"); REQUIRE(x, "x"); REQUIRE(out, "out"); REQUIRE(acts, "acts");
  if (n < 0) return set_error(CRNERF_ERR_SHAPE, "mlp_forward_train_mixed: negative n");
  if (int rc = require_tensors("mlp_forward_train_mixed", tensors)) return rc;
  return launch_mlp_forward_train_mixed(to_tensors(tensors), packed, x, out, acts, (long)n, (hipStream_t)stream);
}

int crnerf_mlp_backward_mixed_f32(const float* const* tensors, const void* packed, const float* x, const float* out, const float* d_out,
                                  const void* acts, void* scratch, float* const* grads, int64_t n, void* stream) {
  if (n == 0) return 0;
  REQUIRE(tensors, "tensors"); REQUIRE(packed, "packed"); REQUIRE(x, "x"); REQUIRE(out, "out"); REQUIRE(d_out, "d_out"); REQUIRE(acts, "acts");
  REQUIRE(scratch, "scratch"); REQUIRE(grads, "grads");
  if (!all_set2(tensors, grads, CRNERF_MLP_TENSORS)) return set_error(CRNERF_ERR_NULL, "mlp_backward_mixed: a tensor / gradient pointer is NULL");
  return launch_mlp_backward_mixed(to_tensors(tensors), packed, x, out, d_out, acts, scratch, grads, (long)n, (hipStream_t)stream);
}

int crnerf_mlp_backward_mixed_ex_f32(const float* const* tensors, const void* packed, const float* out, const float* d_out, const void* acts,
                                     void* scratch, float* const* grads, int64_t n, int acts_layout, void* stream) {
  if (n == 0) return 0;
  REQUIRE(tensors, "tensors"); REQUIRE(packed, "packed"); REQUIRE(out, "out"); REQUIRE(d_out, "d_out"); REQUIRE(acts, "acts");
  REQUIRE(scratch, "scratch"); REQUIRE(grads, "grads");
  if (acts_layout != CRNERF_MIXED_ACTS_GEMM && acts_layout != CRNERF_MIXED_ACTS_FUSED) return set_error(CRNERF_ERR_CONFIG, "mlp_backward_mixed_ex: unknown acts_layout");
  if (!all_set2(tensors, grads, CRNERF_MLP_TENSORS)) return set_error(CRNERF_ERR_NULL, "mlp_backward_mixed_ex: a tensor / gradient pointer is NULL");
  return launch_mlp_backward_mixed(to_tensors(tensors), packed, nullptr, out, d_out, acts, scratch, grads, (long)n, (hipStream_t)stream, acts_layout);
}

int crnerf_render_rays_train_bf16(const crnerf_render_args* a, void* acts_coarse, void* acts_fine, float* raw_coarse, float* raw_fine,
                                  void* stream) {
  return render_rays_train(a, {acts_coarse, acts_fine, raw_coarse, raw_fine}, stream, Core::BF16_PAIR);
}

int crnerf_render_rays_train_f32(const crnerf_render_args* a, void* acts_coarse, void* acts_fine, float* raw_coarse, float* raw_fine,
                                 void* stream) {
  return render_rays_train(a, {acts_coarse, acts_fine, raw_coarse, raw_fine}, stream, Core::F32);
}

size_t crnerf_packed_mlp_t_x3_bytes(void) { return PACKEDXT_BYTES; }

int crnerf_pack_mlp_weights_t_x3(const float* const* tensors, void* packed, void* stream) {
  return pack_entry("pack_mlp_weights_t_x3", tensors, packed, stream, launch_pack_mlp_x3t);
}

int crnerf_mlp_backward_x3_f32(const void* packed_t_x3, const float* x, const float* out, const float* d_out, const void* acts, void* scratch,
                               float* const* grads, int64_t n, int flags, void* stream) {
  if (n == 0) return 0;
  if (int rc = check_backward_args("mlp_backward_x3", flags, CRNERF_BWD_WGRAD_BF16 | CRNERF_BWD_WGRAD_BF16X3, packed_t_x3, x, out, d_out, acts, scratch, grads)) return rc;
  return launch_mlp_backward(nullptr, x, out, d_out, (const float*)acts, scratch, grads, (long)n, (hipStream_t)stream, flags, packed_t_x3);
}

size_t crnerf_packed_mlp_t_h2_bytes(void) { return PACKEDHT_BYTES; }

int crnerf_pack_mlp_weights_t_h2(const float* const* tensors, void* packed, void* stream) {
  return pack_entry("pack_mlp_weights_t_h2", tensors, packed, stream, launch_pack_mlp_h2t);
}

int crnerf_mlp_backward_h2_f32(const void* packed_t_h2, const void* packed_t_x3, const float* x, const float* out, const float* d_out, const void* acts,
                               void* scratch, float* const* grads, int64_t n, int flags, void* stream) {
  if (n == 0) return 0;
  if (int rc = check_backward_args("mlp_backward_h2", flags, CRNERF_BWD_WGRAD_BF16 | CRNERF_BWD_WGRAD_BF16X3 | CRNERF_BWD_WGRAD_F16X2, packed_t_h2, x, out, d_out, acts,
                                   scratch, grads)) return rc;
  // a PHASE_WGRAD call carries no packs; the non-null marker keeps the f16x2 mode (its range words are in the scratch)
  const void* h2 = packed_t_h2 ? packed_t_h2 : (const void*)scratch;
  return launch_mlp_backward(nullptr, x, out, d_out, (const float*)acts, scratch, grads, (long)n, (hipStream_t)stream, flags, packed_t_x3, h2);
}

size_t crnerf_packed_mlp_x3_bytes(void) { return PACKEDX_BYTES; }

int crnerf_pack_mlp_weights_x3(const float* const* tensors, void* packed, void* stream) {
  return pack_entry("pack_mlp_weights_x3", tensors, packed, stream, launch_pack_mlp_x3);
}

int crnerf_mlp_forward_f32x3(const void* packed, const float* x, float* out, int64_t n, int sigma_only, void* stream) {
  return forward_entry("mlp_forward_f32x3", packed, x, out, n, [&](long P) { return launch_mlp_forward_x3(packed, x, out, P, sigma_only, (hipStream_t)stream, 0); });
}

int crnerf_render_rays_f32x3(const crnerf_render_args* a, void* stream) { return render_entry(a, stream, RENDER_RAYS, Core::X3); }

size_t crnerf_packed_mlp_h2_bytes(void) { return PACKEDH_BYTES; }

int crnerf_pack_mlp_weights_h2(const float* const* tensors, void* packed, void* stream) {
  return pack_entry("pack_mlp_weights_h2", tensors, packed, stream, [](const MlpTensors& t, void* p, hipStream_t st) { return launch_pack_mlp_h2(t, p, st); });
}

int crnerf_pack_mlp_weights_h2_async(const float* const* tensors, void* packed, void* stream) {
  return pack_entry("pack_mlp_weights_h2_async", tensors, packed, stream,
                    [](const MlpTensors& t, void* p, hipStream_t st) { return launch_pack_mlp_h2(t, p, st, /*check=*/false); });
}

int crnerf_pack_h2_status(const void* packed_h2, void* stream) {
  REQUIRE(packed_h2, "packed_h2");
  return pack_h2_status(packed_h2, (hipStream_t)stream);
}

int crnerf_mlp_forward_f32h2(const void* packed, const float* x, float* out, int64_t n, int sigma_only, void* stream) {
  return forward_entry("mlp_forward_f32h2", packed, x, out, n, [&](long P) { return launch_mlp_forward_h2(packed, x, out, P, sigma_only, (hipStream_t)stream, 0); });
}

int crnerf_render_rays_f32x3_repair(const crnerf_render_args* a, void* stream) { return render_entry(a, stream, RENDER_RAYS, Core::X3_REPAIR); }
int crnerf_mlp_forward_f32x3_repair(const void* packed, const float* x, float* out, int64_t n, int sigma_only, void* stream) {
  return forward_entry("mlp_forward_f32x3_repair", packed, x, out, n, [&](long P) { return launch_mlp_forward_x3(packed, x, out, P, sigma_only, (hipStream_t)stream, 1); });
}
int crnerf_render_rays_f32h2(const crnerf_render_args* a, void* stream) { return render_entry(a, stream, RENDER_RAYS, Core::H2); }

int crnerf_render_rays_train_f32x3(const crnerf_render_args* a, void* acts_coarse, void* acts_fine, float* raw_coarse, float* raw_fine, void* stream) {
  return render_rays_train(a, {acts_coarse, acts_fine, raw_coarse, raw_fine}, stream, Core::X3);
}

int crnerf_render_rays_train_f32h2(const crnerf_render_args* a, void* acts_coarse, void* acts_fine, float* raw_coarse, float* raw_fine, void* stream) {
  return render_rays_train(a, {acts_coarse, acts_fine, raw_coarse, raw_fine}, stream, Core::H2);
}

int crnerf_render_rays_train_f32x3_repair(const crnerf_render_args* a, void* acts_coarse, void* acts_fine, float* raw_coarse, float* raw_fine, void* stream) {
  return render_rays_train(a, {acts_coarse, acts_fine, raw_coarse, raw_fine}, stream, Core::X3_REPAIR);
}

size_t crnerf_packed_mlp_bf16_bytes(void) { return PACKEDB_BYTES; }

int crnerf_pack_mlp_weights_bf16(const float* const* tensors, void* packed, void* stream) {
  return pack_entry("pack_mlp_weights_bf16", tensors, packed, stream, launch_pack_mlp_bf16);
}

int crnerf_mlp_forward_bf16(const void* packed, const float* x, float* out, int64_t n, int sigma_only, void* stream) {
  return forward_entry("mlp_forward_bf16", packed, x, out, n, [&](long P) { return launch_mlp_forward_bf16p(packed, x, out, P, sigma_only, (hipStream_t)stream); });
}

// include/crnerf_geometry.h: the density query.  A launcher sees a point count in [1, 2^31 - 1] and no NULL pointer.
int crnerf_sigma_points_f32(const void* packed, const float* xyz, float* sigma, int64_t n, void* stream) {
  return sigma_points_entry(packed, xyz, sigma, n, [&](long P) { return launch_sigma_points16(packed, xyz, sigma, P, (hipStream_t)stream); });
}
int crnerf_sigma_points_bf16(const void* packed, const float* xyz, float* sigma, int64_t n, void* stream) {
  return sigma_points_entry(packed, xyz, sigma, n, [&](long P) { return launch_sigma_points_bf16p(packed, xyz, sigma, P, (hipStream_t)stream); });
}
int crnerf_sigma_grid_f32(const void* packed, const float* xs, const float* ys, const float* zs, int32_t nx, int32_t ny, int32_t nz, float* sigma,
                          void* stream) {
  return sigma_grid_entry(packed, xs, ys, zs, nx, ny, nz, sigma, [&] { return launch_sigma_grid16(packed, xs, ys, zs, nx, ny, nz, sigma, (hipStream_t)stream); });
}
int crnerf_sigma_grid_bf16(const void* packed, const float* xs, const float* ys, const float* zs, int32_t nx, int32_t ny, int32_t nz, float* sigma,
                           void* stream) {
  return sigma_grid_entry(packed, xs, ys, zs, nx, ny, nz, sigma, [&] { return launch_sigma_grid_bf16p(packed, xs, ys, zs, nx, ny, nz, sigma, (hipStream_t)stream); });
}

// crnerf_point_features.h (staged beside the sources): the point-feature query.  A launcher sees a point count in [1, 2^31 - 1] and no NULL but sigma.
int crnerf_feature_points_f32(const void* packed, const float* xyz, const float* dirs, float* feature, float* sigma, int64_t n, void* stream) {
  return feature_points_entry(packed, xyz, dirs, feature, n, [&](long P) { return launch_feature_points16(packed, xyz, dirs, feature, sigma, P, (hipStream_t)stream); });
}
int crnerf_feature_points_bf16(const void* packed, const float* xyz, const float* dirs, float* feature, float* sigma, int64_t n, void* stream) {
  return feature_points_entry(packed, xyz, dirs, feature, n, [&](long P) { return launch_feature_points_bf16p(packed, xyz, dirs, feature, sigma, P, (hipStream_t)stream); });
}

size_t crnerf_packed_mlp_f16_bytes(void) { return PACKEDB_BYTES; }

int crnerf_pack_mlp_weights_f16(const float* const* tensors, void* packed, void* stream) {
  return pack_entry("pack_mlp_weights_f16", tensors, packed, stream, launch_pack_mlp_f16);
}

int crnerf_mlp_forward_f16(const void* packed, const float* x, float* out, int64_t n, int sigma_only, void* stream) {
  return forward_entry("mlp_forward_f16", packed, x, out, n, [&](long P) { return launch_mlp_forward_f16p(packed, x, out, P, sigma_only, (hipStream_t)stream); });
}

int crnerf_render_rays_f16(const crnerf_render_args* a, void* stream) { return render_entry(a, stream, RENDER_RAYS, Core::F16_PAIR); }

size_t crnerf_encoder_workspace_bytes(int H, int W) { return encoder_workspace_bytes(H, W); }

int crnerf_encoder_forward_f32(const float* image, int H, int W, const float* const* weights, void* workspace, float* out, void* stream) {
  REQUIRE(image, "image"); REQUIRE(weights, "weights"); REQUIRE(workspace, "workspace"); REQUIRE(out, "out");
  if (!all_set(weights, CRNERF_ENCODER_TENSORS)) return set_error(CRNERF_ERR_NULL, "encoder_forward: a weight pointer is NULL");
  return launch_encoder_forward(image, H, W, weights, workspace, out, (hipStream_t)stream);
}

int crnerf_ray_directions_f32(int H, int W, float fx, float fy, float cx, float cy, float* directions, void* stream) {
  REQUIRE(directions, "directions");
  return launch_ray_directions(fx, fy, cx, cy, H, W, directions, (hipStream_t)stream);
}

int crnerf_rays_from_directions_f32(const float* directions, const float* c2w_host, int64_t n, float* rays_o, float* rays_d, void* stream) {
  if (n == 0) return 0;
  REQUIRE(directions, "directions"); REQUIRE(c2w_host, "c2w"); REQUIRE(rays_o, "rays_o"); REQUIRE(rays_d, "rays_d");
  return launch_rays_from_directions(directions, c2w_host, (long)n, rays_o, rays_d, (hipStream_t)stream);
}

int crnerf_generate_rays_f32(const float* intrinsics_host, const float* c2w_host, int H, int W, float near, float far, float* rays,
                             void* stream) {
  REQUIRE(intrinsics_host, "intrinsics"); REQUIRE(c2w_host, "c2w"); REQUIRE(rays, "rays");
  return launch_generate_rays(intrinsics_host, c2w_host, H, W, near, far, rays, (hipStream_t)stream);
}

int crnerf_generate_rays_fmanorm_f32(const float* intrinsics_host, const float* c2w_host, int32_t H, int32_t W, float near, float far, float* rays,
                                     void* stream) {
  REQUIRE(intrinsics_host, "intrinsics"); REQUIRE(c2w_host, "c2w"); REQUIRE(rays, "rays");
  return launch_generate_rays_fmanorm(intrinsics_host, c2w_host, H, W, near, far, rays, (hipStream_t)stream);
}

int crnerf_crossray_chansum_f32(const float* x, int64_t HW, float* sum64, void* workspace, void* stream) {
  REQUIRE(x, "x"); REQUIRE(sum64, "sum64"); REQUIRE(workspace, "workspace");
  return launch_crossray_chansum(x, (long)HW, sum64, (float*)workspace, (hipStream_t)stream);
}

int crnerf_crossray_gram_f32(const float* x, int64_t HW, const float* mean64, const float* const* cnn, float* gram_sum,
                             void* workspace, void* stream) {
  REQUIRE(x, "x"); REQUIRE(mean64, "mean64"); REQUIRE(cnn, "cnn"); REQUIRE(gram_sum, "gram_sum"); REQUIRE(workspace, "workspace");
  if (!all_set(cnn, 6)) return set_error(CRNERF_ERR_NULL, "crossray_gram: a cnn tensor pointer is NULL");
  CnnTensors w{cnn[0], cnn[1], cnn[2], cnn[3], cnn[4], cnn[5]};
  return launch_crossray_gram(x, (long)HW, mean64, w, gram_sum, (float*)workspace, (hipStream_t)stream);
}

int crnerf_crossray_matrix_f32(const float* gram_sum, double count, const float* fc_w, const float* fc_b, float* out, void* stream) {
  REQUIRE(gram_sum, "gram_sum"); REQUIRE(fc_w, "fc_w"); REQUIRE(fc_b, "fc_b"); REQUIRE(out, "out");
  return launch_crossray_matrix(gram_sum, count, fc_w, fc_b, out, (hipStream_t)stream);
}

int crnerf_crossray_fold_f32(const float* s_matrix, const float* c_matrix, const float* c_mean64, const float* s_mean64,
                             const float* const* lin, float* affine, void* stream) {
  REQUIRE(lin, "lin"); REQUIRE(affine, "affine");
  if (!all_set(lin, 6)) return null_tensor("crossray_fold");
  if (s_matrix) { REQUIRE(c_matrix, "c_matrix"); REQUIRE(c_mean64, "c_mean64"); REQUIRE(s_mean64, "s_mean64"); }
  FoldTensors w{lin[0], lin[1], lin[2], lin[3], lin[4], lin[5]};
  return launch_crossray_fold(s_matrix, c_matrix, c_mean64, s_mean64, w, affine, (hipStream_t)stream);
}

int crnerf_crossray_decode_f32(const float* content, int64_t HW, const float* style, int64_t HWs, const float* const* w,
                               void* workspace, float* rgb, int64_t plane_stride, void* stream) {
  if (HW == 0) return 0;
  REQUIRE(content, "content"); REQUIRE(w, "weights"); REQUIRE(workspace, "workspace"); REQUIRE(rgb, "rgb");
  if (HW < 0 || HWs < 0) return set_error(CRNERF_ERR_SHAPE, "crossray_decode: negative size");
  if (!all_set(w, CRNERF_DECODER_TENSORS)) return set_error(CRNERF_ERR_NULL, "crossray_decode: a weight pointer is NULL");
  const auto d = to_decode_args(content, HW, style, HWs, w, workspace, rgb, plane_stride);
  return launch_crossray_decode(d, (hipStream_t)stream);
}

int crnerf_crossray_decode_sharded_f32(const float* content, int64_t HW_local, const float* style, int64_t HWs, const float* const* w,
                                       int phase, float* xchg, double count_global, void* workspace, float* rgb, int64_t plane_stride,
                                       void* stream) {
  REQUIRE(style, "style"); REQUIRE(w, "weights"); REQUIRE(xchg, "xchg"); REQUIRE(workspace, "workspace");
  if (HW_local < 0 || phase < 0 || phase > 2) return set_error(CRNERF_ERR_SHAPE, "crossray_decode_sharded: bad size or phase");
  if (HW_local > 0) REQUIRE(content, "content");
  if (phase == 2 && HW_local > 0) REQUIRE(rgb, "rgb");
  if (!all_set(w, CRNERF_DECODER_TENSORS)) return set_error(CRNERF_ERR_NULL, "crossray_decode_sharded: a weight pointer is NULL");
  const auto d = to_decode_args(content, HW_local, style, HWs, w, workspace, rgb, plane_stride);
  return launch_crossray_decode_sharded(d, phase, xchg, count_global, (hipStream_t)stream);
}

size_t crnerf_crossray_backward_workspace_bytes(int64_t HW, int64_t HWs) { return crossray_backward_workspace_floats((long)HW, (long)HWs) * sizeof(float); }

int crnerf_crossray_decode_backward_f32(const float* content, int64_t HW, const float* style, int64_t HWs, const float* const* w,
                                        const float* d_rgb, int64_t d_plane_stride, void* workspace, float* d_content, float* d_style,
                                        float* const* grads, void* stream) {
  REQUIRE(content, "content"); REQUIRE(style, "style"); REQUIRE(w, "weights"); REQUIRE(d_rgb, "d_rgb"); REQUIRE(workspace, "workspace");
  REQUIRE(d_content, "d_content"); REQUIRE(d_style, "d_style"); REQUIRE(grads, "grads");
  if (HW <= 0 || HWs <= 0) return set_error(CRNERF_ERR_SHAPE, "crossray_decode_backward: empty grid");
  if (!all_set2(w, grads, CRNERF_DECODER_TENSORS)) return set_error(CRNERF_ERR_NULL, "crossray_decode_backward: a weight or gradient pointer is NULL");
  const auto d = to_decode_args(content, HW, style, HWs, w);     // no workspace, rgb or plane_stride: the backward has its own
  return launch_crossray_decode_backward(d, d_rgb, (long)d_plane_stride, (float*)workspace, d_content, d_style, grads, (hipStream_t)stream);
}

int crnerf_crossray_decode_backward_sharded_f32(const float* content, int64_t HW, const float* style, int64_t HWs, const float* const* w, const float* d_rgb,
                                                int64_t d_plane_stride, void* workspace, float* d_content, float* d_style, float* const* grads, int phase,
                                                const float* fwd_xchg, double count_global, float* xb, void* stream) {
  REQUIRE(content, "content"); REQUIRE(style, "style"); REQUIRE(w, "weights"); REQUIRE(d_rgb, "d_rgb"); REQUIRE(workspace, "workspace");
  REQUIRE(d_content, "d_content"); REQUIRE(d_style, "d_style"); REQUIRE(grads, "grads"); REQUIRE(fwd_xchg, "fwd_xchg"); REQUIRE(xb, "xb");
  if (HW <= 0 || HWs <= 0) return set_error(CRNERF_ERR_SHAPE, "crossray_decode_backward_sharded: empty grid (every rank must hold pixels)");
  if (phase < 0 || phase > 2) return set_error(CRNERF_ERR_CONFIG, "crossray_decode_backward_sharded: phase must be 0, 1 or 2");
  if (!all_set2(w, grads, CRNERF_DECODER_TENSORS)) return set_error(CRNERF_ERR_NULL, "crossray_decode_backward_sharded: a weight or gradient pointer is NULL");
  const auto d = to_decode_args(content, HW, style, HWs, w);     // no workspace, rgb or plane_stride: the backward has its own
  return launch_crossray_decode_backward_sharded(d, d_rgb, (long)d_plane_stride, (float*)workspace, d_content, d_style, grads, phase, fwd_xchg, count_global, xb,
                                                 (hipStream_t)stream);
}

int crnerf_crossray_apply_f32(const float* x, int64_t HW, const float* affine, float* rgb, int64_t plane_stride, void* stream) {
  if (HW == 0) return 0;
  REQUIRE(x, "x"); REQUIRE(affine, "affine"); REQUIRE(rgb, "rgb");
  return launch_crossray_apply(x, (long)HW, affine, rgb, (long)plane_stride, (hipStream_t)stream);
}

// include/crnerf_sweep.h
static_assert(CRNERF_SWEEP_MAX_STYLES == SWEEP_MAX_STYLES && CRNERF_SWEEP_STATS_FLOATS == SWEEP_STATS_FLOATS, "crnerf_sweep.h and crossray.h disagree");

int crnerf_crossray_style_stats_f32(const float* styles, int32_t S, int64_t HWs, int64_t content_HW, const float* const* w, void* workspace,
                                    float* stats, void* stream) {
  if (S < 0 || HWs < 0 || content_HW < 0) return set_error(CRNERF_ERR_SHAPE, "crossray_style_stats: negative size");
  if (S == 0) return 0;
  if (S > CRNERF_SWEEP_MAX_STYLES) return set_error(CRNERF_ERR_SHAPE, "crossray_style_stats: S exceeds CRNERF_SWEEP_MAX_STYLES (split the sweep)");
  REQUIRE(styles, "styles"); REQUIRE(w, "weights"); REQUIRE(workspace, "workspace"); REQUIRE(stats, "stats");
  if (HWs == 0) return set_error(CRNERF_ERR_SHAPE, "crossray_style_stats: empty style grid");
  if (content_HW == 0) return set_error(CRNERF_ERR_SHAPE, "crossray_style_stats: content_HW must be the size of the content grids (>= 1)");
  if (!all_set(w, CRNERF_DECODER_TENSORS)) return set_error(CRNERF_ERR_NULL, "crossray_style_stats: a weight pointer is NULL");
  const CnnTensors snet{w[0], w[1], w[2], w[3], w[4], w[5]};
  return launch_crossray_style_stats(styles, S, (long)HWs, (long)content_HW, snet, w[6], w[7], workspace, stats, (hipStream_t)stream);
}

int crnerf_crossray_decode_multi_f32(const crnerf_sweep_decode_args* a, void* stream) {
  REQUIRE(a, "args");
  if (a->S < 0 || a->HW < 0 || a->style_HW < 0) return set_error(CRNERF_ERR_SHAPE, "crossray_decode_multi: negative size");
  if (a->S == 0 || a->HW == 0) return 0;
  if (a->S > CRNERF_SWEEP_MAX_STYLES) return set_error(CRNERF_ERR_SHAPE, "crossray_decode_multi: S exceeds CRNERF_SWEEP_MAX_STYLES (split the sweep)");
  if (a->out_kind != CRNERF_SWEEP_OUT_F32 && a->out_kind != CRNERF_SWEEP_OUT_U8)
    return set_error(CRNERF_ERR_CONFIG, "crossray_decode_multi: out_kind must be CRNERF_SWEEP_OUT_F32 or CRNERF_SWEEP_OUT_U8");
  REQUIRE(a->content, "content"); REQUIRE(a->stats, "stats"); REQUIRE(a->weights, "weights"); REQUIRE(a->workspace, "workspace"); REQUIRE(a->out, "out");
  if (a->style_HW == 0) return set_error(CRNERF_ERR_SHAPE, "crossray_decode_multi: style_HW must be the size of the style grids behind stats (>= 1)");
  if (!all_set(a->weights, CRNERF_DECODER_TENSORS)) return set_error(CRNERF_ERR_NULL, "crossray_decode_multi: a weight pointer is NULL");
  const bool f32 = a->out_kind == CRNERF_SWEEP_OUT_F32;
  if (f32 && a->plane_stride < a->HW) return set_error(CRNERF_ERR_SHAPE, "crossray_decode_multi: plane_stride is smaller than HW");
  const int64_t image = f32 ? 2 * a->plane_stride + a->HW : 3 * a->HW;
  if (a->S > 1 && a->style_stride < image) return set_error(CRNERF_ERR_SHAPE, "crossray_decode_multi: style_stride makes the images overlap");
  const float* const* w = a->weights;
  SweepArgs d;
  d.content = a->content; d.HW = (long)a->HW; d.stats = a->stats; d.style_HW = (long)a->style_HW; d.S = a->S;
  d.cnet = CnnTensors{w[8], w[9], w[10], w[11], w[12], w[13]}; d.cnet_fc_w = w[14]; d.cnet_fc_b = w[15];
  d.lin = FoldTensors{w[16], w[17], w[18], w[19], w[20], w[21]};
  d.workspace = a->workspace; d.out = a->out; d.out_kind = a->out_kind; d.style_stride = (long)a->style_stride; d.plane_stride = (long)a->plane_stride;
  return launch_crossray_decode_multi(d, (hipStream_t)stream);
}


size_t crnerf_decoder_content_backward_workspace_bytes(int64_t HW) { return content_backward_workspace_floats((long)HW) * sizeof(float); }

int crnerf_decoder_content_backward_f32(const float* content, int64_t HW, const float* rgb_w, const float* rgb, int64_t rgb_plane_stride,
                                        const float* d_rgb, int64_t d_plane_stride, void* workspace, float* d_content, float* d_w, float* d_b,
                                        void* stream) {
  if (HW == 0) return 0;
  REQUIRE(content, "content"); REQUIRE(rgb_w, "rgb_w"); REQUIRE(rgb, "rgb"); REQUIRE(d_rgb, "d_rgb"); REQUIRE(workspace, "workspace");
  REQUIRE(d_content, "d_content"); REQUIRE(d_w, "d_w"); REQUIRE(d_b, "d_b");
  if (HW < 0) return set_error(CRNERF_ERR_SHAPE, "decoder_content_backward: negative HW");
  return launch_content_backward(content, (long)HW, rgb_w, rgb, (long)rgb_plane_stride, d_rgb, (long)d_plane_stride, (float*)workspace, d_content,
                                 d_w, d_b, (hipStream_t)stream);
}

size_t crnerf_encoder_train_saved_bytes(int H, int W) { return encoder_train_saved_bytes(H, W); }
size_t crnerf_encoder_train_scratch_bytes(int H, int W) { return encoder_train_scratch_bytes(H, W); }

int crnerf_encoder_forward_train_f32(const float* image, int H, int W, const float* const* weights, void* saved, float* out, void* stream) {
  REQUIRE(image, "image"); REQUIRE(weights, "weights"); REQUIRE(saved, "saved"); REQUIRE(out, "out");
  if (!all_set(weights, CRNERF_ENCODER_TENSORS)) return set_error(CRNERF_ERR_NULL, "encoder_forward_train: a weight pointer is NULL");
  return launch_encoder_forward_train(image, H, W, weights, saved, out, (hipStream_t)stream);
}

size_t crnerf_encoder_train_band_saved_bytes(int H, int W, int n_out_rows) { return encoder_train_saved_bytes(H, W, n_out_rows * 32); }
size_t crnerf_encoder_train_band_scratch_bytes(int H, int W, int n_out_rows) { return encoder_train_scratch_bytes(H, W, n_out_rows * 32); }

int crnerf_encoder_forward_train_band_f32(const float* image_rows, int H, int W, int H_image, int row0, int o0, int o1, const float* const* weights, void* saved,
                                          float* out, void* stream) {
  REQUIRE(image_rows, "image_rows"); REQUIRE(weights, "weights"); REQUIRE(saved, "saved"); REQUIRE(out, "out");
  if (!all_set(weights, CRNERF_ENCODER_TENSORS)) return set_error(CRNERF_ERR_NULL, "encoder_forward_train_band: a weight pointer is NULL");
  return launch_encoder_forward_train_band(image_rows, H, W, H_image, row0, o0, o1, weights, saved, out, (hipStream_t)stream);
}

int crnerf_encoder_backward_band_f32(int H, int W, int H_image, int row0, int o0, int o1, const float* const* weights, const void* saved, const float* out,
                                     const float* d_out, void* scratch, float* const* grads, float* d_image_rows, void* stream) {
  REQUIRE(weights, "weights"); REQUIRE(saved, "saved"); REQUIRE(out, "out"); REQUIRE(d_out, "d_out"); REQUIRE(scratch, "scratch"); REQUIRE(grads, "grads");
  if (H < 8 || W < 8) return set_error(CRNERF_ERR_SHAPE, "encoder_backward_band: band must be at least 8x8");
  if (!all_set2(weights, grads, CRNERF_ENCODER_TENSORS)) return set_error(CRNERF_ERR_NULL, "encoder_backward_band: a weight or gradient pointer is NULL");
  return launch_encoder_backward_band(H, W, H_image, row0, o0, o1, weights, saved, out, d_out, scratch, grads, d_image_rows, (hipStream_t)stream);
}

int crnerf_encoder_backward_f32(int H, int W, const float* const* weights, const void* saved, const float* out, const float* d_out, void* scratch,
                                float* const* grads, float* d_image, void* stream) {
  REQUIRE(weights, "weights"); REQUIRE(saved, "saved"); REQUIRE(out, "out"); REQUIRE(d_out, "d_out"); REQUIRE(scratch, "scratch"); REQUIRE(grads, "grads");
  if (H < 8 || W < 8) return set_error(CRNERF_ERR_SHAPE, "encoder_backward: image must be at least 8x8");
  if (!all_set2(weights, grads, CRNERF_ENCODER_TENSORS)) return set_error(CRNERF_ERR_NULL, "encoder_backward: a weight or gradient pointer is NULL");
  return launch_encoder_backward(H, W, weights, saved, out, d_out, scratch, grads, d_image, (hipStream_t)stream);
}

static bool to_loss_args(const crnerf_loss_args* a, LossArgs& k, LossScales& sc) {
  k.rgb_c = a->rgb_coarse; k.rgb_f = a->rgb_fine; k.tgt = a->targets; k.mask = a->mask;
  k.a = a->a_embedded; k.a_rand = a->a_embedded_random; k.a_rec = a->a_embedded_random_rec; k.c_wo = a->content_wo; k.c_with = a->content_with;
  k.R = (long)a->n_rays; k.n_a = a->a_embedded ? (long)a->n_a : 0; k.n_rec = a->a_embedded_random_rec ? (long)a->n_rec : 0;
  k.n_c = a->content_wo ? (long)a->n_content : 0;
  k.rc_sr = (long)a->rgb_coarse_row_stride; k.rc_sc = (long)a->rgb_coarse_chan_stride;
  k.rf_sr = (long)a->rgb_fine_row_stride; k.rf_sc = (long)a->rgb_fine_chan_stride;
  k.tg_sr = (long)a->targets_row_stride; k.tg_sc = (long)a->targets_chan_stride;
  k.mse_a = a->mse_on_appearance;
  const double c = a->coef, R = (double)a->n_rays;
  sc.s[0] = k.n_a ? (float)(c * a->weight_kl / (double)k.n_a) : 0.0f;
  sc.s[1] = k.n_rec ? (float)(c * a->weight_rec_a / (double)k.n_rec) : 0.0f;
  sc.s[2] = (float)(c * 0.5 / (3.0 * R));
  sc.s[3] = k.n_c ? (float)(c * a->weight_content / (double)k.n_c) : 0.0f;
  const bool reg = a->mask && a->rgb_fine;                    // r_ms / r_md exist with rgb_fine AND out_mask only (losses.py:67-69)
  sc.s[4] = reg ? (float)(c * a->mask_size_weight / R) : 0.0f;
  sc.s[5] = reg ? (float)(c * a->mask_digit_weight / R) : 0.0f;
  sc.s[6] = a->rgb_fine ? (float)(c * 0.5 / (3.0 * R)) : 0.0f;
  return true;
}

size_t crnerf_loss_workspace_bytes(void) { return loss_workspace_bytes(); }

int crnerf_loss_f32(const crnerf_loss_args* a, float* losses, void* workspace, void* stream) {
  REQUIRE(a, "args"); REQUIRE(losses, "losses"); REQUIRE(workspace, "workspace");
  if (a->n_rays <= 0) return set_error(CRNERF_ERR_SHAPE, "loss: n_rays must be positive");
  REQUIRE(a->rgb_coarse, "rgb_coarse"); REQUIRE(a->targets, "targets");
  if (a->a_embedded_random_rec && !a->a_embedded_random) return set_error(CRNERF_ERR_NULL, "loss: a_embedded_random_rec without a_embedded_random");
  if ((a->content_wo == nullptr) != (a->content_with == nullptr)) return set_error(CRNERF_ERR_NULL, "loss: content_wo and content_with come as a pair");
  LossArgs k; LossScales sc;
  to_loss_args(a, k, sc);
  return launch_loss_forward(k, sc, losses, workspace, (hipStream_t)stream);
}

int crnerf_loss_backward_f32(const crnerf_loss_args* a, const float* upstream, const crnerf_loss_grads* g, void* stream) {
  REQUIRE(a, "args"); REQUIRE(upstream, "upstream"); REQUIRE(g, "grads");
  if (a->n_rays <= 0) return set_error(CRNERF_ERR_SHAPE, "loss_backward: n_rays must be positive");
  REQUIRE(a->rgb_coarse, "rgb_coarse"); REQUIRE(a->targets, "targets");
  LossArgs k; LossScales sc;
  to_loss_args(a, k, sc);
  LossGrads kg{g->d_rgb_coarse, g->d_rgb_fine, g->d_mask, g->d_a_embedded, g->d_a_embedded_random_rec, g->d_content_wo, g->d_content_with};
  return launch_loss_backward(k, sc, upstream, kg, (hipStream_t)stream);
}

// both gathers: the checks, then launch(BatchArgs, hipStream_t)
static int grid_batch_entry(const crnerf_batch_args* a, void* stream, int (*launch)(const BatchArgs&, hipStream_t)) {
  REQUIRE(a, "args");
  if (a->side <= 0) return 0;
  REQUIRE(a->all_rays, "all_rays"); REQUIRE(a->all_rgbs, "all_rgbs"); REQUIRE(a->w_lin, "w_lin"); REQUIRE(a->h_lin, "h_lin");
  REQUIRE(a->rays, "rays"); REQUIRE(a->ts, "ts"); REQUIRE(a->rgbs, "rgbs"); REQUIRE(a->rgb_idx, "rgb_idx"); REQUIRE(a->uv_sample, "uv_sample");
  if (a->img_w <= 0 || a->img_h <= 0 || a->ray_stride < 9) return set_error(CRNERF_ERR_SHAPE, "grid_sample_batch: bad image size or ray_stride < 9");
  BatchArgs k{a->all_rays, (long)a->ray_stride, a->all_rgbs, (long)a->row_offset, a->img_w, a->img_h, a->side, a->w_lin, a->h_lin,
              a->scale, a->h_offset, a->w_offset, a->rays, (long*)a->ts, a->rgbs, (long*)a->rgb_idx, a->uv_sample};
  return launch(k, (hipStream_t)stream);
}

int crnerf_grid_sample_batch_f32(const crnerf_batch_args* a, void* stream) { return grid_batch_entry(a, stream, launch_grid_batch); }
int crnerf_grid_sample_batch_round_f32(const crnerf_batch_args* a, void* stream) { return grid_batch_entry(a, stream, launch_grid_batch_round); }

int crnerf_adam_max_tensors(void) { return ADAM_MAX_TENSORS; }

int crnerf_adam_step_f32(float* params, float* exp_avg, float* exp_avg_sq, const int32_t* blocks, int32_t n_blocks, const float* const* grads,
                         int32_t n_tensors, float step_size, double beta1, double beta2, float eps, float weight_decay, float bias_correction2_sqrt,
                         void* stream) {
  if (n_blocks <= 0) return 0;
  REQUIRE(params, "params"); REQUIRE(exp_avg, "exp_avg"); REQUIRE(exp_avg_sq, "exp_avg_sq"); REQUIRE(blocks, "blocks"); REQUIRE(grads, "grads");
  if (n_tensors <= 0 || n_tensors > ADAM_MAX_TENSORS) return set_error(CRNERF_ERR_SHAPE, "adam_step: n_tensors outside 1 ... crnerf_adam_max_tensors()");
  if (!(bias_correction2_sqrt > 0.0f) || !(eps >= 0.0f)) return set_error(CRNERF_ERR_CONFIG, "adam_step: bias_correction2_sqrt must be positive and eps non-negative");
  // 1 - beta in double, rounded once: what torch.optim.Adam hands its fp32 kernels (1.0f - (float)0.999 is 1.3e-5 relative off)
  const AdamHyper h{step_size, (float)beta1, (float)beta2, eps, weight_decay, bias_correction2_sqrt, (float)(1.0 - beta1), (float)(1.0 - beta2)};
  return launch_adam_step(params, exp_avg, exp_avg_sq, blocks, n_blocks, grads, n_tensors, h, (hipStream_t)stream);
}

static_assert(METRICS_TILE_H == CRNERF_METRICS_TILE_H && METRICS_TILE_W == CRNERF_METRICS_TILE_W, "metrics tile: kernels.h vs crnerf.h");

size_t crnerf_image_metrics_workspace_bytes(int32_t channels, int32_t w, int32_t h) {
  if (channels <= 0 || w <= 0 || h <= 0) return 0;
  return image_metrics_workspace_bytes(channels, w, h);
}

int crnerf_image_metrics_f32(const crnerf_image_metrics_args* a, double* out2, float* ssim_map, void* workspace, void* stream) {
  REQUIRE(a, "args"); REQUIRE(out2, "out2"); REQUIRE(workspace, "workspace");
  REQUIRE(a->pred, "pred"); REQUIRE(a->gt, "gt");
  if (a->channels <= 0 || a->width <= 0 || a->height <= 0) return set_error(CRNERF_ERR_SHAPE, "image_metrics: channels, width and height must be positive");
  if (a->w <= 0 || a->h <= 0) return set_error(CRNERF_ERR_SHAPE, "image_metrics: empty region of interest");
  if (a->w < 2 || a->h < 2) return set_error(-1, "image_metrics: the region of interest must be at least 2x2 (reflect border of the 3x3 window)");
  if (a->x0 < 0 || a->y0 < 0 || a->x0 > a->width - a->w || a->y0 > a->height - a->h)
    return set_error(CRNERF_ERR_SHAPE, "image_metrics: the region of interest leaves the image");
  const long tiles = (long)((a->w + METRICS_TILE_W - 1) / METRICS_TILE_W) * ((a->h + METRICS_TILE_H - 1) / METRICS_TILE_H) * a->channels;
  if (tiles > 0x7fffffffL) return set_error(CRNERF_ERR_SHAPE, "image_metrics: more tiles than one launch holds");
  const MetricsArgs k{a->pred, (long)a->pred_stride_c, (long)a->pred_stride_y, (long)a->pred_stride_x,
                      a->gt, (long)a->gt_stride_c, (long)a->gt_stride_y, (long)a->gt_stride_x,
                      a->channels, a->x0, a->y0, a->w, a->h, a->quantize_pred ? 1 : 0};
  return launch_image_metrics(k, out2, ssim_map, workspace, (hipStream_t)stream);
}

size_t crnerf_lpips_workspace_bytes(int32_t w, int32_t h) {
  if (w < 31 || h < 31 || !lpips_fits_one_launch(w, h)) return 0;
  return lpips_workspace_bytes(w, h);
}

int crnerf_lpips_f32(const crnerf_lpips_args* a, double* out6, float* const* features, void* workspace, void* stream) {
  REQUIRE(a, "args"); REQUIRE(out6, "out6"); REQUIRE(workspace, "workspace");
  REQUIRE(a->pred, "pred"); REQUIRE(a->gt, "gt"); REQUIRE(a->shift, "shift"); REQUIRE(a->scale, "scale");
  for (int l = 0; l < 5; ++l) { REQUIRE(a->conv_w[l], "conv_w[l]"); REQUIRE(a->conv_b[l], "conv_b[l]"); REQUIRE(a->lin[l], "lin[l]"); }
  if (features)
    for (int l = 0; l < 10; ++l) REQUIRE(features[l], "features[l]");
  if (a->width <= 0 || a->height <= 0) return set_error(CRNERF_ERR_SHAPE, "lpips: width and height must be positive");
  if (a->w <= 0 || a->h <= 0) return set_error(CRNERF_ERR_SHAPE, "lpips: empty region of interest");
  if (a->x0 < 0 || a->y0 < 0 || a->x0 > a->width - a->w || a->y0 > a->height - a->h)
    return set_error(CRNERF_ERR_SHAPE, "lpips: the region of interest leaves the image");
  if (a->w < 31 || a->h < 31) return set_error(CRNERF_ERR_SHAPE, "lpips: the region of interest must be at least 31x31 (31 -> 7 -> 3 -> 1 through conv1 and the two pools)");
  if (!lpips_fits_one_launch(a->w, a->h)) return set_error(CRNERF_ERR_SHAPE, "lpips: more patch-matrix blocks than one launch holds");
  for (int l = 0; l < 5; ++l)
    if ((uintptr_t)a->conv_w[l] & 15) return set_error(CRNERF_ERR_SHAPE, "lpips: conv_w[l] must be 16-byte aligned");
  LpipsArgs k{a->pred, (long)a->pred_stride_c, (long)a->pred_stride_y, (long)a->pred_stride_x,
              a->gt, (long)a->gt_stride_c, (long)a->gt_stride_y, (long)a->gt_stride_x,
              a->x0, a->y0, a->w, a->h, a->quantize_pred ? 1 : 0, a->normalize ? 1 : 0, {}, {}, {}, a->shift, a->scale};
  for (int l = 0; l < 5; ++l) { k.conv_w[l] = a->conv_w[l]; k.conv_b[l] = a->conv_b[l]; k.lin[l] = a->lin[l]; }
  return launch_lpips(k, out6, features, workspace, (hipStream_t)stream);
}

static_assert(LANCZOS_TILE_H == CRNERF_LANCZOS_TILE_H && LANCZOS_TILE_W == CRNERF_LANCZOS_TILE_W && LANCZOS_VBLOCK == CRNERF_LANCZOS_VBLOCK,
              "lanczos tiles: kernels.h vs crnerf.h");
static_assert(LANCZOS_U8 == CRNERF_LANCZOS_OUT_U8 && LANCZOS_ROWS == CRNERF_LANCZOS_OUT_ROWS && LANCZOS_CHW == CRNERF_LANCZOS_OUT_CHW &&
              LANCZOS_CHW_SIGNED == CRNERF_LANCZOS_OUT_CHW_SIGNED, "lanczos output modes: kernels.h vs crnerf.h");

size_t crnerf_lanczos_workspace_bytes(int32_t H, int32_t W, int32_t w, int32_t h) {
  if (H < 1 || W < 1 || w < 1 || h < 1) return 0;
  return lanczos_workspace_bytes(H, W, w, h);
}

int crnerf_lanczos_resize_u8(const uint8_t* src, int32_t H, int32_t W, int32_t w, int32_t h, const int32_t* kx, const int32_t* bounds_x, int32_t ksize_x,
                             const int32_t* ky, const int32_t* bounds_y, int32_t ksize_y, int32_t out_mode, void* dst, void* workspace, void* stream) {
  REQUIRE(src, "src"); REQUIRE(dst, "dst");
  if (H < 1 || W < 1 || w < 1 || h < 1) return set_error(CRNERF_ERR_SHAPE, "lanczos_resize: H, W, w and h must be positive");
  if (out_mode < CRNERF_LANCZOS_OUT_U8 || out_mode > CRNERF_LANCZOS_OUT_CHW_SIGNED) return set_error(CRNERF_ERR_CONFIG, "lanczos_resize: unknown output mode");
  if (w != W) {
    REQUIRE(kx, "kx"); REQUIRE(bounds_x, "bounds_x");
    if (ksize_x != lanczos_ksize(W, w)) return set_error(CRNERF_ERR_CONFIG, "lanczos_resize: ksize_x is not the kernel size of W -> w");
    if ((uintptr_t)kx & 15) return set_error(CRNERF_ERR_SHAPE, "lanczos_resize: kx must be 16-byte aligned");
  }
  if (h != H) {
    REQUIRE(ky, "ky"); REQUIRE(bounds_y, "bounds_y");
    if (ksize_y != lanczos_ksize(H, h)) return set_error(CRNERF_ERR_CONFIG, "lanczos_resize: ksize_y is not the kernel size of H -> h");
  }
  if (w != W && h != H) REQUIRE(workspace, "workspace");
  if (!lanczos_fits(H, W, w, h))
    return set_error(CRNERF_ERR_SHAPE, "lanczos_resize: image over 2^31 bytes or 65,535 output rows, or a horizontal downscale whose tile does not fit the LDS (above ~32x)");
  return launch_lanczos_resize(src, H, W, w, h, kx, bounds_x, ksize_x, ky, bounds_y, ksize_y, out_mode, dst, workspace, (hipStream_t)stream);
}

static_assert(RGBA_TILE_H == CRNERF_RGBA_TILE_H && RGBA_TILE_W == CRNERF_RGBA_TILE_W && RGBA_VBLOCK == CRNERF_RGBA_VBLOCK && RGBA_MAX_RECTS == CRNERF_RGBA_MAX_RECTS,
              "rgba tiles: kernels.h vs crnerf_blender.h");
static_assert(RGBA_U8 == CRNERF_RGBA_OUT_U8 && RGBA_ROWS == CRNERF_RGBA_OUT_ROWS && RGBA_CHW == CRNERF_RGBA_OUT_CHW && RGBA_CHW_SIGNED == CRNERF_RGBA_OUT_CHW_SIGNED,
              "rgba output modes: kernels.h vs crnerf_blender.h");

size_t crnerf_rgba_prepare_workspace_bytes(int32_t H, int32_t W, int32_t w, int32_t h) {
  if (H < 1 || W < 1 || w < 1 || h < 1) return 0;
  return rgba_workspace_bytes(H, W, w, h);
}

int crnerf_rgba_prepare_u8(const crnerf_rgba_prepare_args* a, void* stream) {
  static const char who[] = "rgba_prepare";
  REQUIRE(a, "args"); REQUIRE(a->src, "src"); REQUIRE(a->dst, "dst");
  if (a->H < 1 || a->W < 1 || a->w < 1 || a->h < 1) return fail(CRNERF_ERR_SHAPE, who, "H, W, w and h must be positive");
  if (a->out_mode < CRNERF_RGBA_OUT_U8 || a->out_mode > CRNERF_RGBA_OUT_CHW_SIGNED) return fail(CRNERF_ERR_CONFIG, who, "unknown output mode");
  if (a->w != a->W) {
    REQUIRE(a->kx, "kx"); REQUIRE(a->bounds_x, "bounds_x");
    if (a->ksize_x != lanczos_ksize(a->W, a->w)) return fail(CRNERF_ERR_CONFIG, who, "ksize_x is not the kernel size of W -> w");
    if ((uintptr_t)a->kx & 15) return fail(CRNERF_ERR_SHAPE, who, "kx must be 16-byte aligned");
  }
  if (a->h != a->H) {
    REQUIRE(a->ky, "ky"); REQUIRE(a->bounds_y, "bounds_y");
    if (a->ksize_y != lanczos_ksize(a->H, a->h)) return fail(CRNERF_ERR_CONFIG, who, "ksize_y is not the kernel size of H -> h");
  }
  if (a->n_rects < 0 || a->n_rects > CRNERF_RGBA_MAX_RECTS) return fail(CRNERF_ERR_SHAPE, who, "n_rects outside 0 ... CRNERF_RGBA_MAX_RECTS");
  if (a->n_rects > 0) {
    REQUIRE(a->rects, "rects"); REQUIRE(a->colors, "colors");
    for (int i = 0; i < a->n_rects; ++i)
      if (a->rects[4 * i + 2] < a->rects[4 * i] || a->rects[4 * i + 3] < a->rects[4 * i + 1])
        return fail(CRNERF_ERR_SHAPE, who, "a rectangle with x1 < x0 or y1 < y0");
  }
  if ((uintptr_t)a->src & 3) return fail(CRNERF_ERR_SHAPE, who, "src must be 4-byte aligned");
  if (a->out_mode == CRNERF_RGBA_OUT_U8 && ((uintptr_t)a->dst & 3)) return fail(CRNERF_ERR_SHAPE, who, "a uint8 dst must be 4-byte aligned");
  if (a->w != a->W && a->h != a->H) {
    REQUIRE(a->workspace, "workspace");
    if ((uintptr_t)a->workspace & 3) return fail(CRNERF_ERR_SHAPE, who, "workspace must be 4-byte aligned");
  }
  if (!rgba_fits(a->H, a->W, a->w, a->h))
    return fail(CRNERF_ERR_SHAPE, who, "image over 2^31 bytes or 65,535 output rows, or a horizontal downscale whose tile does not fit the LDS (above ~33x)");
  const RgbaPrepare k{a->src, a->H, a->W, a->w, a->h, a->kx, a->bounds_x, a->ksize_x, a->ky, a->bounds_y, a->ksize_y, a->n_rects, a->rects, a->colors,
                      a->lut, a->out_mode, a->dst, a->valid_mask, a->workspace};
  return launch_rgba_prepare(k, (hipStream_t)stream);
}

// a percentile argument the comparisons below may be trusted with: not NaN, not infinite (this unit is compiled with -fno-honor-nans)
static bool finite_bits(double v) {
  uint64_t b;
  memcpy(&b, &v, sizeof b);
  return (b & 0x7FF0000000000000ull) != 0x7FF0000000000000ull;
}

size_t crnerf_scene_bounds_workspace_bytes(int32_t n_images, int32_t n_points) {
  if (n_images < 1 || n_points < 0) return 0;
  return scene_bounds_workspace_bytes(n_images, n_points);
}

int crnerf_scene_bounds_f64(const double* xyz, int32_t n_points, const double* w2c_row2, int32_t n_images, double q_lo, double q_hi, double* nears,
                            double* fars, int32_t* counts, void* workspace, void* stream) {
  if (n_images < 1) return set_error(CRNERF_ERR_SHAPE, "scene_bounds: n_images must be positive");
  if (n_points < 0) return set_error(CRNERF_ERR_SHAPE, "scene_bounds: negative n_points");
  if (n_points > 0) REQUIRE(xyz, "xyz");
  REQUIRE(w2c_row2, "w2c_row2"); REQUIRE(nears, "nears"); REQUIRE(fars, "fars"); REQUIRE(counts, "counts");
  if (!finite_bits(q_lo) || !finite_bits(q_hi) || q_lo < 0.0 || q_lo > 100.0 || q_hi < 0.0 || q_hi > 100.0)
    return set_error(CRNERF_ERR_CONFIG, "scene_bounds: a percentile outside [0, 100]");
  if (q_lo > q_hi) return set_error(CRNERF_ERR_CONFIG, "scene_bounds: q_lo above q_hi");
  if (scene_bounds_workspace_bytes(n_images, n_points) > 0) REQUIRE(workspace, "workspace");
  return launch_scene_bounds(xyz, n_points, w2c_row2, n_images, q_lo / 100.0, q_hi / 100.0, nears, fars, counts, workspace, (hipStream_t)stream);
}

static int to_geom(const crnerf_conv_geom* a, ConvGeom& g) {
  if (a->cin <= 0 || a->cout <= 0 || a->H <= 0 || a->W <= 0 || a->k <= 0 || a->stride <= 0 || a->dil <= 0 || a->pad < 0)
    return set_error(CRNERF_ERR_SHAPE, "conv2d: non-positive geometry");
  if (a->depthwise && a->cin != a->cout) return set_error(CRNERF_ERR_SHAPE, "conv2d: depth-wise needs cin == cout");
  const int Ho = (a->H + 2 * a->pad - a->dil * (a->k - 1) - 1) / a->stride + 1, Wo = (a->W + 2 * a->pad - a->dil * (a->k - 1) - 1) / a->stride + 1;
  if (Ho <= 0 || Wo <= 0) return set_error(CRNERF_ERR_SHAPE, "conv2d: empty output");
  g = ConvGeom{a->cin, a->cout, a->H, a->W, Ho, Wo, a->k, a->stride, a->pad, a->dil, a->depthwise ? 1 : 0};
  return 0;
}

int crnerf_conv2d_f32(const crnerf_conv_geom* geom, const float* x, const float* w, float* y, void* stream) {
  REQUIRE(geom, "geom"); REQUIRE(x, "x"); REQUIRE(w, "w"); REQUIRE(y, "y");
  ConvGeom g;
  if (int e = to_geom(geom, g)) return e;
  return launch_cg_conv_forward(g, x, w, y, (hipStream_t)stream);
}

int crnerf_conv2d_backward_f32(const crnerf_conv_geom* geom, const float* x, const float* w, const float* d_y, float* d_x, float* d_w, void* stream) {
  REQUIRE(geom, "geom"); REQUIRE(x, "x"); REQUIRE(w, "w"); REQUIRE(d_y, "d_y"); REQUIRE(d_w, "d_w");
  ConvGeom g;
  if (int e = to_geom(geom, g)) return e;
  return launch_cg_conv_backward(g, x, w, d_y, d_x, d_w, (hipStream_t)stream);
}

int crnerf_bn_prelu_f32(const float* x, const float* gamma, const float* beta, const float* alpha, float* mean, float* invstd, float* var_unbiased,
                        float* y, int C, int64_t HW, float eps, int training, void* stream) {
  REQUIRE(x, "x"); REQUIRE(gamma, "gamma"); REQUIRE(beta, "beta"); REQUIRE(alpha, "alpha"); REQUIRE(mean, "mean"); REQUIRE(invstd, "invstd"); REQUIRE(y, "y");
  if (training) REQUIRE(var_unbiased, "var_unbiased");
  if (C <= 0 || HW <= 0 || HW > (1 << 30)) return set_error(CRNERF_ERR_SHAPE, "bn_prelu: C and HW must be positive");
  return launch_cg_bn_prelu_forward(x, gamma, beta, alpha, mean, invstd, var_unbiased, y, C, (int)HW, eps, training, (hipStream_t)stream);
}

int crnerf_bn_prelu_train_f32(const float* x, const float* gamma, const float* beta, const float* alpha, float* mean, float* invstd, float* var_unbiased,
                              float* y, float* running_mean, float* running_var, int64_t* num_batches_tracked, float momentum, int C, int64_t HW, float eps,
                              void* stream) {
  REQUIRE(x, "x"); REQUIRE(gamma, "gamma"); REQUIRE(beta, "beta"); REQUIRE(alpha, "alpha"); REQUIRE(mean, "mean"); REQUIRE(invstd, "invstd"); REQUIRE(y, "y");
  REQUIRE(var_unbiased, "var_unbiased"); REQUIRE(running_mean, "running_mean"); REQUIRE(running_var, "running_var");
  if (C <= 0 || HW <= 0 || HW > (1 << 30)) return set_error(CRNERF_ERR_SHAPE, "bn_prelu_train: C and HW must be positive");
  if (!(momentum >= 0.0f && momentum <= 1.0f)) return set_error(CRNERF_ERR_CONFIG, "bn_prelu_train: momentum must be in [0, 1]");
  return launch_cg_bn_prelu_forward(x, gamma, beta, alpha, mean, invstd, var_unbiased, y, C, (int)HW, eps, 1, (hipStream_t)stream, running_mean, running_var,
                                    (long long*)num_batches_tracked, momentum);
}

int crnerf_bn_prelu_backward_f32(const float* x, const float* gamma, const float* beta, const float* alpha, const float* mean, const float* invstd,
                                 const float* d_y, float* d_x, float* d_gamma, float* d_beta, float* d_alpha, int C, int64_t HW, int training,
                                 void* stream) {
  REQUIRE(x, "x"); REQUIRE(gamma, "gamma"); REQUIRE(beta, "beta"); REQUIRE(alpha, "alpha"); REQUIRE(mean, "mean"); REQUIRE(invstd, "invstd");
  REQUIRE(d_y, "d_y"); REQUIRE(d_x, "d_x"); REQUIRE(d_gamma, "d_gamma"); REQUIRE(d_beta, "d_beta"); REQUIRE(d_alpha, "d_alpha");
  if (C <= 0 || HW <= 0 || HW > (1 << 30)) return set_error(CRNERF_ERR_SHAPE, "bn_prelu_backward: C and HW must be positive");
  return launch_cg_bn_prelu_backward(x, gamma, beta, alpha, mean, invstd, d_y, d_x, d_gamma, d_beta, d_alpha, C, (int)HW, training, (hipStream_t)stream);
}

int crnerf_avgpool3s2_f32(const float* in, float* out, int C, int H, int W, int backward, void* stream) {
  REQUIRE(in, "in"); REQUIRE(out, "out");
  if (C <= 0 || H <= 0 || W <= 0) return set_error(CRNERF_ERR_SHAPE, "avgpool3s2: non-positive shape");
  return launch_cg_avgpool(in, out, C, H, W, backward, (hipStream_t)stream);
}

int crnerf_fglo_f32(const float* x, const float* w1, const float* b1, const float* w2, const float* b2, float* stats, float* y, int C, int R, int64_t HW,
                    void* stream) {
  REQUIRE(x, "x"); REQUIRE(w1, "w1"); REQUIRE(b1, "b1"); REQUIRE(w2, "w2"); REQUIRE(b2, "b2"); REQUIRE(stats, "stats"); REQUIRE(y, "y");
  if (C <= 0 || R <= 0 || HW <= 0 || HW > (1 << 22)) return set_error(CRNERF_ERR_SHAPE, "fglo: non-positive shape");
  return launch_cg_fglo_forward(x, w1, b1, w2, b2, stats, y, C, R, (int)HW, (hipStream_t)stream);
}

int crnerf_fglo_backward_f32(const float* x, const float* w1, const float* w2, const float* stats, const float* d_y, float* scratch, float* d_x,
                             float* d_w1, float* d_b1, float* d_w2, float* d_b2, int C, int R, int64_t HW, void* stream) {
  REQUIRE(x, "x"); REQUIRE(w1, "w1"); REQUIRE(w2, "w2"); REQUIRE(stats, "stats"); REQUIRE(d_y, "d_y"); REQUIRE(scratch, "scratch"); REQUIRE(d_x, "d_x");
  REQUIRE(d_w1, "d_w1"); REQUIRE(d_b1, "d_b1"); REQUIRE(d_w2, "d_w2"); REQUIRE(d_b2, "d_b2");
  if (C <= 0 || C > 256 || R <= 0 || R > 64 || HW <= 0 || HW > (1 << 22)) return set_error(CRNERF_ERR_SHAPE, "fglo_backward: bad shape");
  return launch_cg_fglo_backward(x, w1, w2, stats, d_y, scratch, d_x, d_w1, d_b1, d_w2, d_b2, C, R, (int)HW, (hipStream_t)stream);
}

int crnerf_bilinear_gather_f32(const float* in, int h, int w, int Ho, int Wo, const int64_t* idx, int64_t n, int sigmoid, float* out, void* stream) {
  if (n == 0) return 0;
  REQUIRE(in, "in"); REQUIRE(out, "out");
  if (h <= 0 || w <= 0 || Ho <= 0 || Wo <= 0 || n < 0) return set_error(CRNERF_ERR_SHAPE, "bilinear_gather: non-positive shape");
  if (!idx && n != (int64_t)Ho * Wo) return set_error(CRNERF_ERR_SHAPE, "bilinear_gather: idx == NULL means every output pixel (n = Ho*Wo)");
  return launch_cg_bilinear(in, (const long*)idx, out, (long)n, h, w, Ho, Wo, sigmoid, (hipStream_t)stream);
}

int crnerf_bilinear_gather_backward_f32(const float* out, const float* d_out, int h, int w, int Ho, int Wo, const int64_t* idx, int64_t n, int sigmoid,
                                        float* d_in, void* stream) {
  REQUIRE(d_in, "d_in");
  if (h <= 0 || w <= 0 || Ho <= 0 || Wo <= 0 || n < 0) return set_error(CRNERF_ERR_SHAPE, "bilinear_gather_backward: non-positive shape");
  if (n > 0) { REQUIRE(d_out, "d_out"); if (sigmoid) REQUIRE(out, "out"); }
  if (!idx && n != (int64_t)Ho * Wo) return set_error(CRNERF_ERR_SHAPE, "bilinear_gather_backward: idx == NULL means every output pixel");
  return launch_cg_bilinear_backward(out, d_out, (const long*)idx, d_in, (long)n, h, w, Ho, Wo, sigmoid, (hipStream_t)stream);
}

int crnerf_cgnet_param_count(void) { return CGNET_PARAMS; }
int crnerf_cgnet_bn_count(void) { return CGNET_BNS; }
size_t crnerf_cgnet_arena_bytes(int32_t cin, int32_t H, int32_t W) {
  if (cin <= 0 || H <= 0 || W <= 0) return 0;
  return cgnet_arena_floats(cin, H, W) * sizeof(float);
}

static int cgnet_args(const char* who, int32_t cin, int32_t H, int32_t W, const float* const* params) {
  if (cin <= 0 || H < 1 || W < 1 || (long)H * W > (1L << 24)) return set_error(CRNERF_ERR_SHAPE, "cgnet: image must be cin >= 1 channels of 1 ... 2^24 pixels");
  REQUIRE(params, "params");
  if (!all_set(params, CGNET_PARAMS)) return set_error(CRNERF_ERR_NULL, who);
  return 0;
}

int crnerf_cgnet_forward_train_f32(const float* image, int32_t cin, int32_t H, int32_t W, const float* const* params, float* const* running_mean,
                                   float* const* running_var, int64_t* const* num_batches_tracked, float momentum, float eps, void* saved,
                                   float* mask, void* stream) {
  REQUIRE(image, "image"); REQUIRE(saved, "saved"); REQUIRE(mask, "mask"); REQUIRE(running_mean, "running_mean"); REQUIRE(running_var, "running_var");
  if (int rc = cgnet_args("cgnet_forward_train: a params[] entry is NULL", cin, H, W, params)) return rc;
  if (!all_set2(running_mean, running_var, CGNET_BNS)) return set_error(CRNERF_ERR_NULL, "cgnet_forward_train: a running_mean / running_var entry is NULL");
  if (!(eps > 0.0f) || !(momentum >= 0.0f && momentum <= 1.0f)) return set_error(CRNERF_ERR_CONFIG, "cgnet_forward_train: eps must be positive and momentum in [0, 1]");
  const CgNetArgs a{cin, H, W, params, running_mean, running_var, (long long* const*)num_batches_tracked, momentum, eps};
  return launch_cgnet_forward_train(a, image, (float*)saved, mask, (hipStream_t)stream);
}

int crnerf_cgnet_backward_f32(const float* image, int32_t cin, int32_t H, int32_t W, const float* const* params, const void* saved, const float* mask,
                              const float* d_mask, void* scratch, float* const* grads, void* stream) {
  REQUIRE(image, "image"); REQUIRE(saved, "saved"); REQUIRE(mask, "mask"); REQUIRE(d_mask, "d_mask"); REQUIRE(scratch, "scratch"); REQUIRE(grads, "grads");
  if (int rc = cgnet_args("cgnet_backward: a params[] entry is NULL", cin, H, W, params)) return rc;
  if (!all_set(grads, CGNET_PARAMS)) return set_error(CRNERF_ERR_NULL, "cgnet_backward: a grads[] entry is NULL");
  const CgNetArgs a{cin, H, W, params, nullptr, nullptr, nullptr, 0.0f, 1e-3f};
  return launch_cgnet_backward(a, image, (const float*)saved, mask, d_mask, (float*)scratch, grads, (hipStream_t)stream);
}

}  // extern "C"

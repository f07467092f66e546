/* Companion header of include/crnerf.h: the appearance sweep -- one content grid decoded under S styles -- exported from the same
 * libcrnerf_hip.so.  It lives beside crnerf.h only so that crnerf.h and what pins it stay byte for byte as they were.  Conventions (device
 * pointers, `stream`, error codes, crnerf_last_error) are those of crnerf.h; crnerf_abi_version() is unchanged.
 *
 * crnerf_crossray_decode_f32 reads the content grid three times per style (channel sums, Gram, apply) and works out the style's statistics on
 * every call.  The sums and the Gram belong to the content alone and the style's statistics to the style alone, so a sweep splits the call:
 *
 *   crnerf_crossray_style_stats_f32   once per sweep : S style grids -> stats[S][CRNERF_SWEEP_STATS_FLOATS]
 *                                                      stats[s] = the style's channel mean (64 floats), then its 32 x 32 matrix fc(Gram / HWs) (1024)
 *   crnerf_crossray_decode_multi_f32  once per frame : the content's sums, Gram and matrix (the single decode's kernels and block plan), S folds in
 *                                                      one launch, and ONE apply pass that loads every pixel row once and writes S images
 *
 * Image s is BIT-IDENTICAL to crnerf_crossray_decode_f32(content, HW, styles + s*HWs*64, HWs, ...) (tests/test_gpu_sweep.py).
 *   The single decode sums its partial Grams in one of two orders: grids of <= 4096 pixels on BOTH sides take the one-launch reduction, anything
 * else the two-launch one.  The stats therefore belong to one side of that switch: build them with the content_HW they will be used with (any
 * content_HW on the same side gives the same bits), and hand the style grid's size back as style_HW so the content's half takes the same side.
 *
 * `weights` = the HOST array of CRNERF_DECODER_TENSORS device pointers of crnerf_crossray_decode_f32; `workspace` = crnerf_crossray_workspace_bytes()
 * bytes (the single decode's workspace is large enough for a sweep).
 *
 * Returns: 0 for S == 0 (both) or HW == 0 (decode): nothing is enqueued.  CRNERF_ERR_NULL for a missing pointer, the field's name in
 * crnerf_last_error.  CRNERF_ERR_SHAPE for a negative size, an empty style grid, S > CRNERF_SWEEP_MAX_STYLES (split the sweep into several
 * calls) or a stride that makes images overlap.  CRNERF_ERR_CONFIG for an unknown out_kind. */
#ifndef CRNERF_SWEEP_H
#define CRNERF_SWEEP_H

#include "crnerf.h"

#ifdef __cplusplus
extern "C" {
#endif

#define CRNERF_SWEEP_MAX_STYLES 16      /* the S folded maps stay in LDS: 16 x 196 floats = 12.5 KiB */
#define CRNERF_SWEEP_STATS_FLOATS 1088  /* mean[64] | matrix[1024] */

#define CRNERF_SWEEP_OUT_F32 0 /* float out[s*style_stride + c*plane_stride + px]: the sigmoid output, planar like crnerf_crossray_decode_f32's rgb */
#define CRNERF_SWEEP_OUT_U8 1  /* unsigned char out[s*style_stride + 3*px + c] = (unsigned char)(fminf(fmaxf(v, 0), 1) * 255.0f), a NaN stores 0:
                                * S frames [H,W,3]; plane_stride is ignored */

typedef struct crnerf_sweep_decode_args {
  const float* content;         /* [HW][64] */
  int64_t HW;
  const float* stats;           /* [S][CRNERF_SWEEP_STATS_FLOATS] of crnerf_crossray_style_stats_f32, dense */
  int64_t style_HW;             /* pixels of the style grids the stats were made from */
  int32_t S;
  int32_t out_kind;             /* CRNERF_SWEEP_OUT_* */
  const float* const* weights;  /* HOST array of CRNERF_DECODER_TENSORS device pointers */
  void* workspace;
  void* out;
  int64_t style_stride;         /* elements of `out` between two styles' images */
  int64_t plane_stride;         /* CRNERF_SWEEP_OUT_F32: floats between two colour planes (>= HW) */
} crnerf_sweep_decode_args;

/* styles[S][HWs][64] -> stats[S][CRNERF_SWEEP_STATS_FLOATS]; content_HW >= 1: the size of the content grids the stats will be used with. */
int crnerf_crossray_style_stats_f32(const float* styles, int32_t S, int64_t HWs, int64_t content_HW, const float* const* weights,
                                    void* workspace, float* stats, void* stream);
int crnerf_crossray_decode_multi_f32(const crnerf_sweep_decode_args* args, void* stream);

#ifdef __cplusplus
}
#endif

#endif

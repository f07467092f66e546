/* Companion header of include/crnerf.h: the entry points of the Blender dataset path, exported from the same
 * libcrnerf_hip.so.  It lives beside crnerf.h only so that crnerf.h and what pins it stay byte for byte as they were when this path was
 * added; folding the two is moving these declarations to the end of crnerf.h.  Conventions (device pointers, `stream`, error codes,
 * crnerf_last_error) are those of crnerf.h.
 *
 * -------- RGBA preparation: what datasets/blender_mask_grid_sample.py does on the host between the decoded RGBA PNG and the tensors of the
 * dataset -- add_perturbation (:16-36), PIL.Image.resize(img_wh, Image.LANCZOS) of an RGBA image, ToTensor, the blend on white (:106-110,
 * :174-178) and Normalize(0.5, 0.5) -- as one chain, bit for bit.  A pixel is one dword: R, G, B, A in ascending bytes.
 *
 * Load stage, applied to every source pixel (y, x) by whichever pass reads the source:
 *   1. occluders: n_rects <= CRNERF_RGBA_MAX_RECTS rectangles, rects[i] = inclusive (x0, y0, x1, y1) in source pixels (any part outside the
 *      image is clipped away), colors[i] = (R, G, B).  The LAST rectangle with x0 <= x <= x1 and y0 <= y <= y1 replaces the pixel by its
 *      colour with alpha 255 -- ImageDraw.rectangle(((x0, y0), (x1, y1)), fill=rgb) on an RGBA image, drawn in order.
 *   2. colour table: lut[c][v], c = R, G, B, replaces each colour byte; alpha is untouched.  The table of add_perturbation's 'color' is
 *      (uint8)(255 * clip(s[c] * (v / 255.0) + b[c], 0, 1)) in float64, built on the host (crnerf_amd.datasets.blender.perturbation_params).
 *   3. premultiply, ONLY when a resize runs (w != W or h != H): t = c * a + 128, c' = ((t >> 8) + t) >> 8; alpha is kept (Pillow's
 *      RGBA -> RGBa conversion).
 * Lanczos passes: those of crnerf_lanczos_resize_u8 (crnerf.h states the table and the arithmetic) on the four channels of the
 * premultiplied image: acc = 2^21 + sum in[xmin + x] * k[x] in int32, out = clamp(acc >> 22, 0, 255), an arithmetic shift; the horizontal
 * pass first, when w != W, into a uint8 image [H, w, 4] in the workspace; the vertical pass second, when h != H; a pass that keeps its size
 * is skipped.  The tables are crnerf_amd.datasets.images.lanczos_coeffs'; windows are clamped, no table content makes the kernels leave src.
 * Store stage, applied by the last pass that runs (a pointwise kernel when none does):
 *   1. un-premultiply, ONLY when a resize ran: c unchanged for a == 0 or a == 255, else c = min(255, (255 * c') / a), an integer division
 *      (Pillow's RGBa -> RGBA conversion).
 *   2. out_mode:
 *      CRNERF_RGBA_OUT_U8          uint8 [h, w, 4]
 *      CRNERF_RGBA_OUT_ROWS        fp32 [h*w, 3]: x = c / 255, a = alpha / 255 (correctly rounded divisions), x * a + (1 - a) -- the product,
 *                                  the difference and the sum each rounded to fp32 on its own, never contracted
 *      CRNERF_RGBA_OUT_CHW         fp32 [3, h, w] of the same blend
 *      CRNERF_RGBA_OUT_CHW_SIGNED  fp32 [3, h, w]: (v - 0.5) / 0.5 of that
 *      each bit-identical to the torch expression evaluated on the host.
 *   3. valid_mask, when not NULL: uint8 [h*w] = alpha > 0, alongside any out_mode.
 * Identity: with w == W and h == H nothing is premultiplied -- a pixel with alpha 1 ... 254 keeps its colour bytes, as Image.resize returns
 * a copy when the size does not change.
 * src: [H, W, 4] uint8, contiguous, device, 4-byte aligned.  kx / bounds_x, ky / bounds_y, ksize_x / ksize_y: as crnerf_lanczos_resize_u8
 * (those of a skipped pass are not read and may be NULL; kx 16-byte aligned).  rects: int32 [n_rects, 4] and colors: uint8 [n_rects, 3]
 * are HOST arrays, read before the call returns (NULL allowed when n_rects == 0).  lut: uint8 [3, 256], device, or NULL.  dst is a base
 * pointer: a slice of a larger buffer is a valid target.  workspace: crnerf_rgba_prepare_workspace_bytes(H, W, w, h) bytes, H * w * 4 when
 * both passes run, else 0 (then it may be NULL).  Nothing is allocated; asynchronous on `stream`.
 * Returns CRNERF_ERR_NULL for a missing pointer; CRNERF_ERR_CONFIG for an unknown out_mode or a ksize that is not that of its size pair;
 * CRNERF_ERR_SHAPE, before any launch, for a size < 1, n_rects outside [0, CRNERF_RGBA_MAX_RECTS], a rectangle with x1 < x0 or y1 < y0, a
 * kx that is not 16-byte aligned, an image (source, intermediate or output) of 2^31 bytes or more, more than 65,535 output rows, or a
 * horizontal downscale beyond what one tile's rows fit in 64 KiB of LDS: with s = W / w the tile takes at most 1952 s + 544 bytes, so
 * W / w up to 33 always fits (800 -> 25 does). */
#ifndef CRNERF_BLENDER_H
#define CRNERF_BLENDER_H

#include "crnerf.h"

#ifdef __cplusplus
extern "C" {
#endif

#define CRNERF_RGBA_OUT_U8 0
#define CRNERF_RGBA_OUT_ROWS 1
#define CRNERF_RGBA_OUT_CHW 2
#define CRNERF_RGBA_OUT_CHW_SIGNED 3
#define CRNERF_RGBA_MAX_RECTS 16
#define CRNERF_RGBA_TILE_H 8      /* rows x output columns of one workgroup of the horizontal pass ...                     */
#define CRNERF_RGBA_TILE_W 32
#define CRNERF_RGBA_VBLOCK 256    /* ... and pixels of an output row of one workgroup of the vertical pass: sizes worth testing */
typedef struct {
  const uint8_t* src;
  int32_t H, W, w, h;
  const int32_t* kx; const int32_t* bounds_x;
  const int32_t* ky; const int32_t* bounds_y;
  int32_t ksize_x, ksize_y;
  int32_t n_rects, out_mode;
  const int32_t* rects; const uint8_t* colors;
  const uint8_t* lut;
  void* dst; uint8_t* valid_mask; void* workspace;
} crnerf_rgba_prepare_args;
size_t crnerf_rgba_prepare_workspace_bytes(int32_t H, int32_t W, int32_t w, int32_t h);
int crnerf_rgba_prepare_u8(const crnerf_rgba_prepare_args* args, void* stream);

/* -------- the Blender batcher's gather: crnerf_grid_sample_batch_f32 (crnerf.h) with the one arithmetic step in which
 * BlenderDataset.__getitem__ (datasets/blender_mask_grid_sample.py:139-163) differs from the Phototourism one: the pixel of a lattice node is
 * (h_sb * img_h).round() / (w_sb * img_w).round(), torch's round = half to even = rintf, where the other takes floorf.  Same struct, same
 * checks, same outputs. */
int crnerf_grid_sample_batch_round_f32(const crnerf_batch_args* args, void* stream);

/* -------- the Blender dataset's rays: crnerf_generate_rays_f32 (crnerf.h; same arguments, same checks, same rays[H*W, 8]) with the one
 * step that makes rays_d bit-identical to the reference's get_rays (datasets/ray_utils.py:44-45) as torch evaluates it on an FMA host:
 *   rotated[k] = fma(dz, R[k][2], fma(dy, R[k][1], dx * R[k][0]))        -- directions @ c2w[:, :3].T; crnerf_generate_rays_f32 does the same
 *   n = sqrt(fma(r2, r2, fma(r1, r1, r0 * r0)))                           -- torch.norm(rays_d, dim=-1): acc = fma(d, d, acc) from 0, in order
 *   rays_d = rotated / n, a correctly rounded division per component.
 * crnerf_generate_rays_f32 sums the three squares without fma and stays within 2 ulp of this; BlenderDataset's all_rays / rays are
 * recorded from the reference itself (tests/golden/g19_blender.npz) and held to equality, which needs this entry point. */
int crnerf_generate_rays_fmanorm_f32(const float* intrinsics_host, const float* c2w_host, int32_t H, int32_t W, float near, float far, float* rays,
                                     void* stream);

#ifdef __cplusplus
}
#endif

#endif

/* mvlt_hip_ingest.h -- the device-side image ingest entry points of libmvlt_hip.so (docs/ingest.md), added beside the C ABI of mvlt_hip.h (version 8) and the
 * additions of mvlt_hip_ext.h, mvlt_hip_ema.h, mvlt_hip_plan.h, mvlt_hip_opt.h, mvlt_hip_lamb.h and mvlt_hip_loss.h, whose lists of prototypes and versions stay
 * as they are.  What a data loader decoded -- uint8 pixels, one source rectangle per sample -- becomes the clean fp32 image AND its grid-masked copy in one pass;
 * mvlt_grid_mask_apply (mvlt_hip.h) remains the fp32-in path and is not touched.
 *
 * Same library, same conventions as mvlt_hip.h: the caller owns every buffer (device pointers unless said otherwise), everything is asynchronous on the
 * hipStream_t passed as `void* stream` (NULL = default stream), no syncs, no allocation; returns 0 on success, <0 on error, mvlt_last_error() has the text.
 * A binding compares mvlt_ingest_version() with the MVLT_INGEST_VERSION it was written against (mvlt_amd/_lib.py INGEST_VERSION) before it calls anything here.
 */
#ifndef MVLT_HIP_INGEST_H
#define MVLT_HIP_INGEST_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

/* Version of this header: bumped whenever a signature below changes or one is added.
 *   1: mvlt_image_ingest(), mvlt_image_ingest_resize(), mvlt_flip_flags() */
#define MVLT_INGEST_VERSION 1
int mvlt_ingest_version(void);

/* The largest downscale factor mvlt_image_ingest_resize accepts: a rectangle of h x w pixels is resampled to H x W only if h <= 8 H and w <= 8 W (upscaling is
 * unbounded).  A workgroup keeps the horizontally filtered source rows under its band of 8 output rows in LDS: at factor f those are at most 9 f + 1 rows
 * (73 at f = 8) of 32 columns x 3 channels fp32 = 28 KB, next to a 12.5 KB staging buffer for 16 raw source rows of at most 33 f + 1 pixels -- 41 KB per
 * workgroup, three workgroups per 160 KB CU.  Factor 8 covers 1360-pixel sources down to 224. */
#define MVLT_INGEST_MAX_FACTOR 8
/* no side of a slab or of an output exceeds this (the integer filter weights and their sums then stay far inside int32) */
#define MVLT_INGEST_MAX_SIDE 16384

/* image[b,c,y,x] = table[c][src pixel] -- uint8 in, fp32 (B,3,H,W) out, no resampling.
 *   src     uint8, (B,H,W,3) for layout 0, (B,3,H,W) for layout 1
 *   table   fp32[3][256]: the caller computes the 256 values of each channel once, the way its host transform would (v / 255, then (. - mean) / std), so the
 *           output equals that transform bit for bit by construction; the kernel stages it in LDS
 *   masked, flags: both NULL, or masked fp32 (B,3,H,W) and flags uint8 (B, H/patch, W/patch): the same pass also writes
 *           masked[b,c,y,x] = flags[b, y/patch, x/patch] ? fill : image[b,c,y,x]      (the contract of mvlt_grid_mask_apply; H, W multiples of patch)
 * 16-byte stores and 4-byte loads when W is a multiple of 4, src is 4-byte and image / masked are 16-byte aligned; element by element otherwise.
 * B == 0 returns 0 without a launch. */
int mvlt_image_ingest(const uint8_t* src, int layout, const float* table, float* image, float* masked, const uint8_t* flags, int B, int H, int W, int patch,
                      float fill, void* stream);

/* The same outputs from a padded uint8 slab src (B,Hmax,Wmax,3), with each sample's rectangle rects[b] = {y0, x0, h, w} (int32, inside the slab, h, w >= 1)
 * resampled to (H, W) by the antialiased triangle filter, separable, horizontal pass then vertical pass (the geometry of Pillow's Image.resize(BILINEAR)); the
 * intermediate stays in fp32.  Along one axis, for output index i, input index x relative to the rectangle, input size n and output size m:
 *     d = (2x+1) m - (2i+1) n,   D = 2 max(n, m),   weight(i, x) = max(0, D - |d|),   taps = the x in [0, n) of positive weight
 * (integers: no float comparison decides a tap, nothing outside the rectangle is ever read).  Horizontal: (sum w_k v_k) / (sum w_k), both sums exact in int32,
 * one fp32 division.  Vertical: the same weights on the fp32 intermediates, accumulated in fp32 by ascending source row, divided by the integer weight sum, then
 * divided by 255.  norm: NULL, or fp32[6] = {mean[3], std[3]} (device): (. - mean[c]) / std[c] afterwards, in that order.  At n == m the weights are {0, D, 0} and the
 * output is bit-identical to mvlt_image_ingest with the table built from the same formulas.  flip: NULL or uint8[B]; a set flip[b] mirrors the output columns of
 * sample b (image and masked alike; flags are indexed by the OUTPUT position).
 *   rects_host: a HOST copy of rects, required: it is what the checks below read (no sync); the kernel reads the device copy and skips a sample whose device
 *   rectangle would fail them.
 * Refused before any launch: a rectangle that leaves the slab or has h < 1 or w < 1; h > MVLT_INGEST_MAX_FACTOR * H or w > MVLT_INGEST_MAX_FACTOR * W; H or W that is
 * not a multiple of patch when flags are given; a side above MVLT_INGEST_MAX_SIDE; B above 65535. */
int mvlt_image_ingest_resize(const uint8_t* src, int Hmax, int Wmax, const int* rects, const int* rects_host, const uint8_t* flip, const float* norm, float* image,
                             float* masked, const uint8_t* flags, int B, int H, int W, int patch, float fill, void* stream);

/* flip[b] = ((draw >> 8) < threshold), draw = word 0 of the Philox4x32-10 draw (seed, sample0 + b, element 0, stream 6) -- the generator and counter layout of
 * mvlt_grid_mask_flags / mvlt_token_mask (streams 0, 1, 2, 4, 5 are theirs and the step's) -- and threshold = round(p * 2^24) (to nearest, ties to even), p in [0, 1]. */
int mvlt_flip_flags(uint8_t* flip, int B, float p, uint64_t seed, uint64_t sample0, void* stream);

#ifdef __cplusplus
}
#endif
#endif

/* mvlt_hip_ema.h -- the weight-EMA entry points of libmvlt_hip.so, added beside the C ABI of mvlt_hip.h (version 8) and the additions of mvlt_hip_ext.h
 * (version 1), whose lists of prototypes and versions stay as they are.
 *
 * Same library, same conventions as mvlt_hip.h: the caller owns every buffer (device pointers, contiguous), everything is asynchronous on the hipStream_t
 * passed as `void* stream` (NULL = default stream), no syncs, no allocation; returns 0 on success, <0 on error, mvlt_last_error() has the text.
 * A binding compares mvlt_ema_version() with the MVLT_EMA_VERSION it was written against (mvlt_amd/_lib.py EMA_VERSION) before it calls anything here.
 */
#ifndef MVLT_HIP_EMA_H
#define MVLT_HIP_EMA_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

/* Version of this header: bumped whenever a signature below changes or one is added.
 *   1: mvlt_ema_update(), mvlt_ema_update_buffers() */
#define MVLT_EMA_VERSION 1
int mvlt_ema_version(void);

/* Exponential moving average of the model's weights.  Replaces timm.utils.ModelEma (imported at reference main_vl.py:16, the `model_ema = None` of
 * main_vl.py:295 is where one would be built, the commented `'model_ema': get_state_dict(model_ema)` of main_vl.py:452 where it would be saved), whose
 * update(model) the training loop calls after every optimizer step (reference engine_grid_masking.py:130-131) and which runs
 *   ema_v.copy_(ema_v * decay + (1. - decay) * model_v)
 * once per state_dict entry: three ATen launches per tensor.  Here the parameters of both models are flat buffers and one launch does them all.
 *
 * mvlt_ema_update: for i in [0, n):  ema[i] = fadd_rn(fmul_rn(ema[i], decay), fmul_rn(p[i], one_minus_decay))
 *   Three fp32 operations, each rounded to nearest even on its own (never contracted into an FMA): the bits of timm's formula evaluated in fp32 with
 *   decay and 1 - decay rounded to fp32 by the caller.  Both factors come by value: nothing is read from the device but ema, p and the mask.
 *   ema_bf16 (nullable): receives the bf16 (round to nearest even) of the new ema[i] in the same pass -- the bits mvlt_cast_bf16 (mvlt_hip.h) gives for the
 *   new values, so the averaged model's next forward needs no cast of its own.
 *   mask (nullable): one byte per element.  MVLT_ADAMW_FROZEN (2, mvlt_hip.h: the byte mvlt_adamw_step gives a frozen element) = the element is left alone:
 *   neither ema[i] nor ema_bf16[i] is written, and ema[i] / p[i] reach nothing.  Every other value = update.  A 16-byte vector whose four bytes are all
 *   frozen costs the four mask bytes only.
 *   n % 4 == 0; ema, p 16-byte aligned, ema_bf16 8-byte aligned, mask 4-byte aligned.  0 <= decay <= 1 and 0 <= one_minus_decay <= 1 (NaN is refused).
 *   n == 0 returns 0 without a launch.
 * mvlt_ema_update_buffers: the module buffers (BatchNorm running statistics and counters) of the two models, all in one launch.
 *   table: int64[n_tensors][4] ON THE DEVICE, one row per tensor = {dst address, src address, numel, kind}; workgroup t handles tensor t.
 *   kind 0: fp32, dst[i] = fadd_rn(fmul_rn(dst[i], decay), fmul_rn(src[i], one_minus_decay)) as above;  kind 1: int64, dst[i] = src[i] (a counter --
 *   num_batches_tracked -- is copied, not averaged);  any other kind: the row is skipped.  Scalar accesses: a tensor may start at any address aligned
 *   for its element type and have any length (numel <= 0: nothing happens).
 *   n_tensors == 0 returns 0 without a launch. */
int mvlt_ema_update(float* ema, const float* p, void* ema_bf16, long n, float decay, float one_minus_decay,
                    const uint8_t* mask /* [n], MVLT_ADAMW_FROZEN = leave alone */, void* stream);
int mvlt_ema_update_buffers(const int64_t* table /* int64[n_tensors][4], device */, int n_tensors, float decay, float one_minus_decay, void* stream);

#ifdef __cplusplus
}
#endif
#endif

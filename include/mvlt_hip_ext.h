/* mvlt_hip_ext.h -- entry points of libmvlt_hip.so added beside the C ABI of mvlt_hip.h (whose version 8 and whose list of prototypes stay as they are).
 *
 * Same library, same conventions as mvlt_hip.h: the caller owns every buffer (device pointers, contiguous), everything is asynchronous on the hipStream_t
 * passed as `void* stream` (NULL = default stream), no syncs, no allocation; returns 0 on success, <0 on error, mvlt_last_error() has the text.
 * A binding compares mvlt_ext_version() with the MVLT_EXT_VERSION it was written against (mvlt_amd/_lib.py EXT_VERSION) before it calls anything here.
 */
#ifndef MVLT_HIP_EXT_H
#define MVLT_HIP_EXT_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

/* Version of this header: bumped whenever a signature below changes or one is added.
 *   1: mvlt_step_gate(), mvlt_adamw_step_gated() */
#define MVLT_EXT_VERSION 1
int mvlt_ext_version(void);

/* Skip the optimizer step on non-finite gradients, decided on the device.  Replaces what timm's NativeScaler (a torch.cuda.amp.GradScaler) does inside
 * loss_scaler(total_loss, optimizer, clip_grad=max_norm, ...) at reference engine_grid_masking.py:126-127 (main_vl.py:309): a backward pass that left Inf or
 * NaN in a gradient does not step the optimizer.  The reference's own check of the loss (engine_grid_masking.py:116-120) only prints a warning and carries on;
 * the GradScaler reads its found-inf flag back to the host.  Here nothing is read back: the decision stays in a 4-float device record that the AdamW kernel obeys.
 *
 * mvlt_step_gate: one workgroup folds the n_partials (1..1024) partial sums of squares that mvlt_grad_sumsq (mvlt_hip.h) stored, through the same device
 *   function and in the same order as mvlt_clip_coef, and writes
 *     out[0] = total_norm = grad_scale * sqrt(sum)       the bits mvlt_clip_coef's out[0] has on the same partials (grad_scale: the factor still owed to g)
 *     out[1] = coefficient: exactly 0 when total_norm is Inf or NaN; min(1, max_norm / (total_norm + 1e-6)) when it is finite and max_norm > 0
 *              (torch.nn.utils.clip_grad_norm_'s formula); exactly 1 when it is finite and max_norm <= 0 (no clipping asked for)
 *     out[2] = ok: 1.0f when total_norm is finite, else 0.0f
 *     out[3] = 0 (reserved)
 *   then counters[0] += ok, counters[1] += !ok (applied / skipped steps; int[2] on the device, zeroed once by the caller and kept from step to step).
 *   Plain loads and stores by one thread, no atomics: launches on one stream are ordered.  A sum of squares that overflows fp32 (one |g| above about
 *   1.8e19) counts as non-finite, as torch's fp32 norm of the same gradients reports inf.
 * mvlt_adamw_step_gated: mvlt_adamw_step (mvlt_hip.h: same p, g, m, v, p_bf16, n, hp, decay_mask) with the gate in the place of gscale_dev.  Every thread
 *   loads gate[2] first; when it is 0 the thread returns before any load or store of p, g, m, v, p_bf16 or decay_mask: the step did not happen.  When it
 *   is 1 the results are those of mvlt_adamw_step(..., gscale_dev = &gate[1]) in every bit, frozen mask bytes (MVLT_ADAMW_FROZEN) included.
 *   n % 4 == 0; gate is required. */
int mvlt_step_gate(const float* partials, int n_partials, float grad_scale, float max_norm, float* out /* fp32[4], device */,
                   int* counters /* int[2], device, persistent */, void* stream);
int mvlt_adamw_step_gated(float* p, const float* g, float* m, float* v, void* p_bf16, long n, const float* hp,
                          const uint8_t* decay_mask /* [n] 0 / 1 / MVLT_ADAMW_FROZEN */, const float* gate /* fp32[4] of mvlt_step_gate */, void* stream);

#ifdef __cplusplus
}
#endif
#endif

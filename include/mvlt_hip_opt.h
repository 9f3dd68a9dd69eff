/* mvlt_hip_opt.h -- the per-group AdamW entry point of libmvlt_hip.so, added beside the C ABI of mvlt_hip.h (version 8) and the additions of mvlt_hip_ext.h,
 * mvlt_hip_ema.h and mvlt_hip_plan.h, whose lists of prototypes and versions stay as they are.
 *
 * Same library, same conventions as mvlt_hip.h: the caller owns every buffer (device pointers, contiguous), everything is asynchronous on the hipStream_t
 * passed as `void* stream` (NULL = default stream), no syncs, no allocation; returns 0 on success, <0 on error, mvlt_last_error() has the text.
 * A binding compares mvlt_opt_version() with the MVLT_OPT_VERSION it was written against (mvlt_amd/_lib.py OPT_VERSION) before it calls anything here.
 */
#ifndef MVLT_HIP_OPT_H
#define MVLT_HIP_OPT_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

/* Version of this header: bumped whenever a signature below changes or one is added.
 *   1: mvlt_adamw_step_groups() */
#define MVLT_OPT_VERSION 1
int mvlt_opt_version(void);

/* The group byte of an element no launch steps: a frozen parameter (requires_grad=False) or an alignment gap.  What MVLT_ADAMW_FROZEN (mvlt_hip.h) is to
 * mvlt_adamw_step's decay mask. */
#define MVLT_OPT_FROZEN 255
#define MVLT_OPT_MAX_GROUPS 254

/* torch.optim.AdamW over a flat fp32 buffer whose elements belong to parameter groups with a learning rate and a weight decay of their own -- what
 * timm's create_optimizer (reference main_vl.py:308) builds when it is given a layer decay or a list of groups, and what engine_grid_masking.py:126 then
 * steps, tensor by tensor.  One launch; mvlt_adamw_step (mvlt_hip.h) and mvlt_adamw_step_gated (mvlt_hip_ext.h) stay as they are and remain the
 * launch for one learning rate.
 *
 * p, g, m, v, p_bf16 (nullable), n: as for mvlt_adamw_step.
 * hp (device, fp32[8]): the row of mvlt_adamw_step, {lr, beta1, beta2, eps, weight_decay, 1-beta1^t, 1-beta2^t, grad_scale}; slots 0 and 4 are IGNORED.
 * table (device, fp32[n_groups][2]): {lr, weight_decay} of group k at table[2k], table[2k + 1].  1 <= n_groups <= MVLT_OPT_MAX_GROUPS.
 * group_of (device, one byte per element):
 *   0 .. n_groups - 1     the element's group.  Its arithmetic is mvlt_adamw_step's for a decay-mask byte of 1 with hp[0] = the group's lr and
 *                         hp[4] = the group's weight decay, in every bit (a weight decay of 0 multiplies p by exactly 1).  The step size lr / (1-beta1^t)
 *                         and the decay factor 1 - lr * weight_decay are formed once per group and workgroup, in LDS, by the same operations.
 *   MVLT_OPT_FROZEN       p, m, v and p_bf16 are NOT written, and g / m / v of the element reach nothing (a NaN or Inf there is harmless).
 *   any other byte        (n_groups .. 254) is treated as MVLT_OPT_FROZEN: nothing outside the table is ever read.
 *   Any four bytes may stand in one 16-byte vector.  A vector whose four bytes are all frozen is skipped after the byte read: no load, no store; one
 *   without a frozen byte is stored as vectors; a mixed one lane by lane.
 * gscale_dev, gate (both nullable, at most one of them): gscale_dev is mvlt_adamw_step's -- a device scalar multiplied into hp[7], the clip coefficient
 *   of mvlt_clip_coef.  gate is mvlt_adamw_step_gated's -- the fp32[4] record of mvlt_step_gate: every thread loads gate[2] first and, when it is 0,
 *   returns before any load or store of p, g, m, v, p_bf16, group_of or table; when it is 1 the results are those of gscale_dev = &gate[1] in every bit.
 * n % 4 == 0; p, g, m, v 16-byte aligned, p_bf16 and table 8-byte aligned, group_of 4-byte aligned.  n == 0 returns 0 without a launch. */
int mvlt_adamw_step_groups(float* p, const float* g, float* m, float* v, void* p_bf16, long n, const float* hp,
                           const uint8_t* group_of /* [n] group index, MVLT_OPT_FROZEN = leave alone */,
                           const float* table /* fp32[n_groups][2] = {lr, weight_decay}, device */, int n_groups,
                           const float* gscale_dev, const float* gate /* fp32[4] of mvlt_step_gate */, void* stream);

#ifdef __cplusplus
}
#endif
#endif

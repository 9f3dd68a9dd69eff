/* mvlt_hip_loss.h -- the label-smoothed / class-weighted cross-entropy entry points of libmvlt_hip.so (docs/loss_options.md), added beside the C ABI of
 * mvlt_hip.h (version 8) and the additions of mvlt_hip_ext.h, mvlt_hip_ema.h, mvlt_hip_plan.h, mvlt_hip_opt.h and mvlt_hip_lamb.h, whose lists of prototypes
 * and versions stay as they are.  mvlt_cross_entropy_fwd / mvlt_cross_entropy_bwd (mvlt_hip.h) remain the plain loss and are not touched.
 *
 * Same library, same conventions as mvlt_hip.h: the caller owns every buffer (device pointers), everything is asynchronous on the hipStream_t passed as
 * `void* stream` (NULL = default stream), no syncs, no allocation; returns 0 on success, <0 on error, mvlt_last_error() has the text.
 * A binding compares mvlt_loss_version() with the MVLT_LOSS_VERSION it was written against (mvlt_amd/_lib.py LOSS_VERSION) before it calls anything here.
 */
#ifndef MVLT_HIP_LOSS_H
#define MVLT_HIP_LOSS_H
#ifdef __cplusplus
extern "C" {
#endif

/* Version of this header: bumped whenever a signature below changes or one is added.
 *   1: mvlt_ce_smooth_fwd(), mvlt_ce_smooth_bwd() */
#define MVLT_LOSS_VERSION 1
int mvlt_loss_version(void);

/* torch.nn.functional.cross_entropy(logits, labels, weight=w, ignore_index=i, label_smoothing=e, reduction="mean") over the rows of an fp32 matrix
 * logits [rows, V] with leading dimension ld >= V (the columns [V, ld) are never read), labels int64 [rows].
 * With p = softmax(x_r), keep_r = [labels[r] != ignore_index], W = sum_c w_c and den = sum_r keep_r w[y_r]  (weight == NULL: w = 1, W = V, den = the row count):
 *     loss         = sum_r keep_r [ (1 - e) w[y_r] (lse_r - x[r, y_r])  +  (e / V) (W lse_r - sum_c w_c x[r, c]) ] / den
 *     dlogits[r,k] = keep_r [ (1 - e) w[y_r] (p_k - [k == y_r])  +  (e / V) (W p_k - w_k) ] gscale / den
 * V is the class count, never ld.  An ignored row adds to neither term and its gradient row is zero.  den is NOT clamped: with weights den < 1 is
 * legitimate; den == 0 (every row ignored) leaves loss_num / den = 0 / 0 to the caller (NaN, as in torch) and gives an all-zero gradient (1 / den is taken as 0).
 *
 * label_smoothing in [0, 1).  weight: NULL or fp32[V].  dtype: the logits' (1 = fp32 is the only one accepted).
 * Outside the contract: a row that holds -inf while e > 0 (torch's loss is +inf there; here the row's smoothing term is inf or NaN).  With e == 0 the -inf
 *   columns of a row are as welcome as in mvlt_cross_entropy_fwd (the smoothing sums are not formed at all) as long as the label is on a finite column.
 * A label outside [0, V) that is not ignore_index reads nothing (torch raises): the loss and the row's gradient are NaN.
 *
 * mvlt_ce_smooth_fwd: two launches.  One workgroup per row reads the row ONCE and writes lse[r] and, for e > 0,
 *   smooth[r] = W lse_r - sum_c w_c x[r, c], accumulated against the pivot x[r, 0] as W ((max - x0) + log sum) - sum_c w_c (x_c - x0): the two products are
 *   ~V |x| each and would cancel to ~V log V in fp32.  (e == 0: smooth is neither written nor read.)  Then ONE workgroup visits the rows in a fixed order and
 *   stores acc[0] = the numerator of the loss, acc[1] = den, acc[2] = W: plain stores, no atomics -- the same input gives the same bits every time, and acc
 *   needs no zeroing.  rows == 0 runs the second launch alone (acc = {0, 0, W}).
 * lse, smooth: fp32[rows]; acc: fp32[3]. */
int mvlt_ce_smooth_fwd(const void* logits, const long* labels, long ignore_index, float label_smoothing, const float* weight, float* lse, float* smooth,
                       float* acc, int rows, int V, int ld, int dtype, void* stream);

/* mvlt_ce_smooth_bwd: one launch, one workgroup per row, from the lse and acc the forward left.  gscale: a DEVICE scalar (the incoming gradient of the loss).
 * dlogits [rows, ldd], ldd >= V, fp32 (out_dtype 1) or bf16 (out_dtype 0, round to nearest even); its padding columns [V, ldd) are written as zeros.
 * 16-byte accesses when logits, dlogits (and weight) are 16-byte aligned and ld, ldd are multiples of 4; element by element otherwise and for the V & 3 tail.
 * rows == 0 returns 0 without a launch. */
int mvlt_ce_smooth_bwd(const void* logits, const long* labels, long ignore_index, float label_smoothing, const float* weight, const float* lse,
                       const float* gscale, const float* acc, void* dlogits, int rows, int V, int ld, int ldd, int dtype, int out_dtype, void* stream);

#ifdef __cplusplus
}
#endif
#endif

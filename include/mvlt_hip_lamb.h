/* mvlt_hip_lamb.h -- the LAMB entry points of libmvlt_hip.so (layer-wise trust ratios over the flat parameter store, docs/lamb.md), added beside the C ABI of
 * mvlt_hip.h (version 8) and the additions of mvlt_hip_ext.h, mvlt_hip_ema.h, mvlt_hip_plan.h and mvlt_hip_opt.h, whose lists of prototypes and versions stay
 * as they are.
 *
 * Same library, same conventions as mvlt_hip.h: the caller owns every buffer (device pointers, contiguous), everything is asynchronous on the hipStream_t
 * passed as `void* stream` (NULL = default stream), no syncs, no allocation; returns 0 on success, <0 on error, mvlt_last_error() has the text.
 * A binding compares mvlt_lamb_version() with the MVLT_LAMB_VERSION it was written against (mvlt_amd/_lib.py LAMB_VERSION) before it calls anything here.
 */
#ifndef MVLT_HIP_LAMB_H
#define MVLT_HIP_LAMB_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

/* Version of this header: bumped whenever a signature below changes or one is added.
 *   1: mvlt_lamb_check_tables(), mvlt_lamb_moments(), mvlt_lamb_fold(), mvlt_lamb_apply() */
#define MVLT_LAMB_VERSION 1
int mvlt_lamb_version(void);

/* LAMB (You et al., "Large Batch Optimization for Deep Learning", as apex's FusedLAMB states it -- what timm 0.3.2's create_optimizer builds for
 * `--opt fusedlamb`, reference main_vl.py:308) for every tensor T of a flat fp32 buffer that trains this step, with lr / wd of T's group:
 *     g = G * gs;   m = b1 m + (1 - b1) g;   v = b2 v + (1 - b2) g g;   u = (m / bc1) / (sqrt(v / bc2) + eps) + wd p
 *     r[T] = ||p||_2 / ||u||_2  if (wd != 0 or ALWAYS_ADAPT) and ||p|| > 0 and ||u|| > 0, else 1;   TRUST_CLIP: r[T] = min(r[T], 1)
 *     p = p - lr r[T] u
 * both norms over T's own elements.  Three launches -- mvlt_lamb_moments, mvlt_lamb_fold, mvlt_lamb_apply, in this order on one stream -- with no atomics,
 * no host read and no scratch beyond two floats per chunk: the same state gives the same bits every time, whatever stands next to T in the buffer.
 *
 * The buffer is described by two tables (device copies for the launches, host copies for mvlt_lamb_check_tables):
 *   tensors  int64[n_tensors][MVLT_LAMB_ROW] = {offset, length, group, frozen, first_chunk, n_chunks}: T occupies elements [offset, offset + length) of the
 *            flat buffers (offset a multiple of 4, tensors ascending and disjoint), takes {lr, wd} from table[group], is left alone when frozen != 0, and
 *            owns the n_chunks = ceil(length / MVLT_LAMB_CHUNK) rows of `chunks` that start at first_chunk (rows of successive tensors follow each other).
 *   chunks   int32[n_chunks][2] = {tensor, k}: workgroup c of mvlt_lamb_moments / mvlt_lamb_apply works on elements
 *            [offset + k CHUNK, offset + min((k + 1) CHUNK, length)) of that tensor and on nothing else -- never on the alignment gap behind it.
 * hp (device, fp32[8]): the row of mvlt_adamw_step, {-, beta1, beta2, eps, -, 1-beta1^t, 1-beta2^t, grad_scale}; slots 0 and 4 are IGNORED.
 * table (device, fp32[n_groups][2]): {lr, weight_decay} of group k, as for mvlt_adamw_step_groups.  1 <= n_groups <= 254.
 * gate (nullable, every launch): the fp32[4] record of mvlt_step_gate.  Every thread loads gate[2] first and returns on 0 before it touches anything else:
 *   p, m, v, p_bf16, partials and ratios keep every bit.
 * Frozen tensors: their chunks return after the table read.  p, m, v, p_bf16 and ratios[T] are not written, nothing of theirs is read.
 * A row of either table that names something outside the buffers (a tensor past n, a group past the table, a chunk past its tensor) makes its workgroup
 * return without a load or a store: mvlt_lamb_check_tables is where such a table is refused with a message. */
#define MVLT_LAMB_CHUNK 16384
#define MVLT_LAMB_ROW 6
#define MVLT_LAMB_ALWAYS_ADAPT 1 /* flags of mvlt_lamb_fold: the trust ratio also where weight_decay == 0 (apex: use_nvlamb) */
#define MVLT_LAMB_TRUST_CLIP 2   /*                          r = min(r, 1) */

/* HOST tables in, nothing launched, no device needed: 0 when the launches below may take their device copies for buffers of n elements, else <0 and the text
 * names the first offending row -- a tensor or chunk that points past n, an offset that is no multiple of 4, tensors that overlap or descend, a group outside
 * [0, n_groups), n_chunks / first_chunk that do not tile `chunks`, a chunk row that is not {its tensor, its index in it}. */
int mvlt_lamb_check_tables(const int64_t* tensors /* HOST */, int n_tensors, const int32_t* chunks /* HOST */, int n_chunks, long n, int n_groups);

/* Launch 1, one workgroup per chunk: reads p, g, m, v, writes m, v (the bits mvlt_adamw_step leaves for the same g, m, v, beta1, beta2, grad scale), and
 * stores partials[2c] = sum p^2, partials[2c + 1] = sum u^2 over the chunk (plain stores; the slots of frozen chunks are not written and not read later).
 * gscale_dev (nullable, not together with gate): a device scalar multiplied into hp[7]; with a gate the factor is gate[1]. */
int mvlt_lamb_moments(const float* p, const float* g, float* m, float* v, long n, const float* hp, const int64_t* tensors, int n_tensors,
                      const int32_t* chunks, int n_chunks, const float* table, int n_groups, float* partials /* fp32[n_chunks][2] */,
                      const float* gscale_dev, const float* gate, void* stream);

/* Launch 2, one workgroup per tensor: sums the tensor's partials in a fixed order and writes ratios[T] (fp32[n_tensors]; readable afterwards, for logging). */
int mvlt_lamb_fold(const float* partials, int n_chunks, const int64_t* tensors, int n_tensors, const float* table, int n_groups, int flags, float* ratios,
                   const float* gate, void* stream);

/* Launch 3, one workgroup per chunk: recomputes u from the m, v and p launch 1 left (the same expressions), writes p = p - lr ratios[T] u and, when p_bf16 is
 * given, the bf16 (round to nearest even) of the new p in the same pass.
 * p, m, v 16-byte aligned, p_bf16 / table / tensors / partials 8-byte aligned, chunks / ratios 4-byte aligned.  n == 0, n_tensors == 0 or n_chunks == 0
 * returns 0 without a launch (all three). */
int mvlt_lamb_apply(float* p, const float* m, const float* v, void* p_bf16, long n, const float* hp, const int64_t* tensors, int n_tensors,
                    const int32_t* chunks, int n_chunks, const float* table, int n_groups, const float* ratios, const float* gate, void* stream);

#ifdef __cplusplus
}
#endif
#endif

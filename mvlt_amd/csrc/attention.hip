// Spatial-reduction attention core for MVLT (gfx950): O = softmax(Q K^T * scale) V, head_dim 64, any number M of keys: the resident kernels
// keep all keys of a head in LDS up to 320 (bf16) / 288 (fp32) keys; past that the key-streamed kernels take over.
// Replaces reference libs/pvlt.py:113-117 (two bmm + softmax that materialise the (B,h,N,M) score tensor).
//
// PVT's spatial reduction keeps M = (H/r)^2 + T small (192 at 256 px, 272 at 384 px) in every stage, so the whole
// K (M x 64) and V^T (64 x M) of one (batch, head) live in LDS for the lifetime of a workgroup and the softmax is
// single-pass: a wave owns 32 queries, computes S^T = K Q^T with v_mfma_f32_32x32x16_bf16 (so each lane holds the
// scores of ONE query: the row reduction is lane-local plus one cross-half shuffle), exponentiates in registers,
// and feeds P^T straight back as the B operand of O^T = V^T P^T.  Nothing but Q, K, V, O and the log-sum-exp
// touches HBM.  fp32 instantiation (exact-f32 MFMA 32x32x2) serves the 1e-3 parity bar.
//
// One translation unit per kernel family, compiled in parallel: attention_fwd.hip (resident forward), attention_fwd2.hip (round-3 bf16 forward), attention_bwd.hip
// (resident fp32 backward), attention_bwd_dma.hip (resident bf16 backward), attention_stream.hip (both key-streamed kernels); attention_common.h holds what more than
// one of them uses.  What to launch is decided in attn_plan.h, a pure host function; this file hands a plan to its family's launch function -- an unknown family is an
// error, never another kernel -- and keeps the C entry points.
#include "attention_common.h"

namespace {

int launch_fwd(const mvlt_attn_args* a, bool streamed, void* stream) {
  mvlt_attn_plan p;
  MVLT_REQUIRE(a, "%s: null pointer", streamed ? "mvlt_sr_attention_fwd_streamed" : "mvlt_sr_attention_fwd");
  if (const int rc = plan_attn_fwd(*a, streamed, p)) return rc;
  switch (p.family) {
    case MVLT_ATTN_FWD: return mvlt_launch_attn_fwd(*a, p, (hipStream_t)stream);
    case MVLT_ATTN_FWD2: return mvlt_launch_attn_fwd2(*a, p, (hipStream_t)stream);
    case MVLT_ATTN_FWD_STREAM: return mvlt_launch_attn_fwd_stream(*a, p, (hipStream_t)stream);
  }
  return attn_no_instantiation("mvlt_sr_attention_fwd", p);
}

int launch_bwd(const mvlt_attn_bwd_args* a, bool streamed, void* stream) {
  mvlt_attn_plan p;
  MVLT_REQUIRE(a, "%s: null pointer", streamed ? "mvlt_sr_attention_bwd_streamed" : "mvlt_sr_attention_bwd");
  if (const int rc = plan_attn_bwd(*a, streamed, p)) return rc;
  switch (p.family) {
    case MVLT_ATTN_BWD: return mvlt_launch_attn_bwd(*a, p, (hipStream_t)stream);
    case MVLT_ATTN_BWD_DMA: return mvlt_launch_attn_bwd_dma(*a, p, (hipStream_t)stream);
    case MVLT_ATTN_BWD_STREAM: return mvlt_launch_attn_bwd_stream(*a, p, (hipStream_t)stream);
  }
  return attn_no_instantiation("mvlt_sr_attention_bwd", p);
}

}  // namespace

extern "C" int mvlt_sr_attention_fwd(const mvlt_attn_args* a, void* stream) { return launch_fwd(a, false, stream); }
extern "C" int mvlt_sr_attention_fwd_streamed(const mvlt_attn_args* a, void* stream) { return launch_fwd(a, true, stream); }
extern "C" int mvlt_sr_attention_bwd(const mvlt_attn_bwd_args* a, void* stream) { return launch_bwd(a, false, stream); }
extern "C" int mvlt_sr_attention_bwd_streamed(const mvlt_attn_bwd_args* a, void* stream) { return launch_bwd(a, true, stream); }

// query chunks of the backward this library would launch with an fp32 dKV (1: the schedule hands it a bf16 dKV instead); 0 for a non-positive shape, no error text
extern "C" int mvlt_sr_attention_bwd_chunks(int B, int H, int N, int M, int dtype) {
  if (B <= 0 || H <= 0 || N <= 0 || M <= 0) return 0;
  mvlt_attn_plan p = {};
  mvlt_attn::choose_bwd(B, H, N, M, dtype == 0 ? 0 : 1, false, false, p);
  return p.nq_chunks;
}

// the plan without the launch (include/mvlt_hip_plan.h): no device is touched
extern "C" int mvlt_attn_plan_sizeof(void) { return (int)sizeof(mvlt_attn_plan); }
extern "C" int mvlt_sr_attention_fwd_plan(const mvlt_attn_args* a, int streamed, mvlt_attn_plan* plan) {
  MVLT_REQUIRE(a && plan, "mvlt_sr_attention_fwd_plan: null argument");
  return plan_attn_fwd(*a, streamed != 0, *plan);
}
extern "C" int mvlt_sr_attention_bwd_plan(const mvlt_attn_bwd_args* a, int streamed, mvlt_attn_plan* plan) {
  MVLT_REQUIRE(a && plan, "mvlt_sr_attention_bwd_plan: null argument");
  return plan_attn_bwd(*a, streamed != 0, *plan);
}
extern "C" int mvlt_attn_plan_name(const mvlt_attn_plan* plan, char* buf, size_t n) {
  MVLT_REQUIRE(plan && buf && n > 0, "mvlt_attn_plan_name: null argument");
  return plan_attn_name(*plan, buf, n);
}

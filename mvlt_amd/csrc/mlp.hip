// Fused MLP kernels for the narrow stages (C = 64 / 128: stage 1 and 2 of PVLT), gfx950.
//
// Reference libs/pvlt.py:65-71 runs fc1 -> GELU -> fc2 as three kernels and round-trips the (tokens x hidden) activation
// through HBM three times (18.4 MB per pair per block in stage 1).  With C = 64/128 the GEMMs have
// K = C: far below the MFMA/HBM ridge, so the hidden activation is the whole cost.  Here a workgroup owns 128 (C=64)
// or 64 (C=128) token rows, keeps their x tile in LDS, and walks the hidden dimension in chunks of 64 units:
//
//   forward  (mode 0):  G_c = gelu(x W1_c^T + b1_c)           producer MFMAs -> bf16 tile in LDS
//                       out += G_c W2[:, c]^T                 consumer MFMAs (accumulators live across chunks)
//                       out = (out + b2) * droppath + residual            (fp32 residual stream)
//   backward (mode 1):  H_c = x W1_c^T + b1_c ; dG_c = dy W2[:, c]        two producers
//                       dH_c = dG_c * gelu'(H_c)                          -> bf16 tile in LDS
//                       dx += dH_c W1_c                                   consumer; dx *= droppath
//
// so the hidden activation never leaves the CU (forward can optionally still store the pre-activation for the unfused
// backward).  Producers are computed transposed (rows = hidden units, columns = tokens) so that each lane ends up with
// four consecutive hidden units of one token: one 8-byte LDS store into the consumer's A-operand tile.
//
// One translation unit per kernel family, compiled in parallel: mlp_fused.hip (the round-2 forward / input-gradient kernel), mlp_pipe.hip (the software-pipelined one),
// mlp_wgrad.hip (both weight-gradient kernels, the activation table and the folds behind the partial tiles); mlp_common.h holds what more than one of them uses.  What to
// launch is decided in mlp_plan.h, a pure host function; this file hands a plan to its family's launch function -- an unknown family is an error, never another kernel --
// and keeps the C entry points.
#include "mlp_common.h"

namespace {

int launch(const char* who, const mvlt_mlp_args& a, const mvlt_mlp_plan& p, void* stream) {
  switch (p.family) {
    case MVLT_MLP_NONE: return MVLT_OK;
    case MVLT_MLP_FUSED: return mvlt_launch_mlp_fused(a, p, (hipStream_t)stream, who);
    case MVLT_MLP_PIPE: return mvlt_launch_mlp_pipe(a, p, (hipStream_t)stream, who);
    case MVLT_MLP_WGRAD:
    case MVLT_MLP_WGRAD2: return mvlt_launch_mlp_wgrad(a, p, (hipStream_t)stream, who);
  }
  return mlp_no_instantiation(who, p);
}

}  // namespace

extern "C" int mvlt_mlp_fwd(const mvlt_mlp_args* a, void* stream) {
  mvlt_mlp_plan p;
  MVLT_REQUIRE(a, "mvlt_mlp_fwd: null pointer");
  if (int e = plan_mlp_fwd(*a, p)) return e;
  return launch("mvlt_mlp_fwd", *a, p, stream);
}

extern "C" int mvlt_mlp_bwd_dx(const mvlt_mlp_args* a, void* stream) {
  mvlt_mlp_plan p;
  MVLT_REQUIRE(a, "mvlt_mlp_bwd_dx: null pointer");
  if (int e = plan_mlp_bwd_dx(*a, p)) return e;
  return launch("mvlt_mlp_bwd_dx", *a, p, stream);
}

extern "C" int mvlt_mlp_bwd_dw(const mvlt_mlp_args* a, void* stream) {
  mvlt_mlp_plan p;
  MVLT_REQUIRE(a, "mvlt_mlp_bwd_dw: null pointer");
  if (int e = plan_mlp_bwd_dw(*a, p)) return e;
  return launch("mvlt_mlp_bwd_dw", *a, p, stream);
}

// the plan without the launch (include/mvlt_hip_plan.h): no device is touched
extern "C" int mvlt_mlp_plan_sizeof(void) { return (int)sizeof(mvlt_mlp_plan); }
extern "C" int mvlt_mlp_fwd_plan(const mvlt_mlp_args* a, mvlt_mlp_plan* plan) {
  MVLT_REQUIRE(a && plan, "mvlt_mlp_fwd_plan: null argument");
  return plan_mlp_fwd(*a, *plan);
}
extern "C" int mvlt_mlp_bwd_dx_plan(const mvlt_mlp_args* a, mvlt_mlp_plan* plan) {
  MVLT_REQUIRE(a && plan, "mvlt_mlp_bwd_dx_plan: null argument");
  return plan_mlp_bwd_dx(*a, *plan);
}
extern "C" int mvlt_mlp_bwd_dw_plan(const mvlt_mlp_args* a, mvlt_mlp_plan* plan) {
  MVLT_REQUIRE(a && plan, "mvlt_mlp_bwd_dw_plan: null argument");
  return plan_mlp_bwd_dw(*a, *plan);
}
extern "C" int mvlt_mlp_plan_name(const mvlt_mlp_plan* plan, char* buf, size_t n) {
  MVLT_REQUIRE(plan && buf && n > 0, "mvlt_mlp_plan_name: null argument");
  return plan_mlp_name(*plan, buf, n);
}

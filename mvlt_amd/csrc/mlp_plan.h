// Host side of the fused-MLP entry points (stages 1-2, C = 64 / 128): argument checks, then the choice of kernel family, template arguments, launch geometry, dynamic LDS
// bytes and, for the weight gradients, the token splits and whether they leave as partial tiles -- a pure function of the argument struct (no HIP call, no global state, no
// launch; plain C++17, compiles with a host compiler alone).  mlp.hip hands a plan to its family's file (mlp_<family>.hip: one case list per family, no shape condition
// there); include/mvlt_hip_plan.h exports the plan, and tests/test_mlp_plan_cpu.py pins it against launches recorded on an MI355X.  Every rule of the dispatch is stated
// HERE, once; DESIGN.md ("MLP dispatch: plan, then launch") has the table of the 12 instantiations.
#pragma once
#include <stdint.h>
#include <stdio.h>
#include "../../include/mvlt_hip_plan.h"
#include "plan_common.h"
#include "mlp_common.h"

namespace mvlt_mlp {

inline bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

// what mvlt_mlp_fwd and mvlt_mlp_bwd_dx check alike
inline int check(const mvlt_mlp_args& a, const char* who) {
  MVLT_REQUIRE((a.x || a.ln_x) && a.w1 && a.wb && a.b1 && (a.out || a.out_op || a.lnb_x), "%s: null pointer", who);
  MVLT_REQUIRE(a.C == 64 || a.C == 128, "%s: C must be 64 or 128 (stage 1 / 2), got %d", who, a.C);
  MVLT_REQUIRE(a.hid > 0 && a.hid % 64 == 0, "%s: hidden size must be a multiple of 64", who);
  MVLT_REQUIRE(!a.row_scale || a.rows_per_scale > 0, "%s: row_scale needs rows_per_scale", who);
  return MVLT_OK;
}

// a size the runtime could only refuse at the launch is refused here, by name
inline int bound(mvlt_mlp_plan& p, const char* who, int hid, size_t lds, long grid) {
  MVLT_REQUIRE(lds <= 160 * 1024, "%s: hid=%d needs %zu B of LDS (>160 KB)", who, hid, lds);
  MVLT_REQUIRE(grid <= 0x7fffffffL, "%s: %ld workgroups", who, grid);
  p.lds = (int)lds;
  p.grid = (int)grid;
  return MVLT_OK;
}

// forward (MODE 0) and input gradient (MODE 1), for checked arguments: a workgroup owns 128 token rows.  The software-pipelined kernel takes every launch it can: it
// stores no pre-activation (nothing in the step asks for one) and its steady state needs an even number >= 4 of 32-unit slices; at C = 128 the input gradient fits
// since the polynomial GELU' (44 B of scratch, 297 us against the round-2 kernel's 339 us).  The round-2 kernel keeps the launches with a pre-activation output or
// hid == 64.
inline int choose(const mvlt_mlp_args& a, int mode, const char* who, mvlt_mlp_plan& p) {
  const bool pipe = !a.h_out && a.hid >= 128;
  p.family = pipe ? MVLT_MLP_PIPE : MVLT_MLP_FUSED;
  p.tp[0] = a.C; p.tp[1] = mode;
  p.block = NT;
  return bound(p, who, a.hid, pipe ? pipe_lds(a.C, mode, a.hid) : fused_lds(a.C, mode, a.hid), ((long)a.M + BM - 1) / BM);
}

// workgroups of the ordered fold of an [N1][N2] output (gemm.hip: 32 groups of 8 elements per 256-thread workgroup)
inline int fold_wgs(long n1, long n2) { return (int)((n1 * n2 / 8 + 31) / 32); }

// weight gradients, for checked arguments: a workgroup owns 128 hidden units (ny of them cover hid) and one of `splits` token ranges of m_per_split rows, whole 64-token
// tiles.  One round of workgroups (2 per CU at C = 64, 1 per CU at C = 128): every extra split costs hid * C * 2 fp32 atomics, or as many bf16 partials to fold.
inline int choose_dw(const mvlt_mlp_args& a, const char* who, mvlt_mlp_plan& p) {
  const int C = a.C, ny = a.hid / 128;
  int splits = ((C == 64 ? 512 : 256) + ny - 1) / ny;
  splits = (splits + 7) / 8 * 8;
  const int mtiles = (int)(((long)a.M + 63) / 64);
  if (splits > mtiles) splits = mtiles;
  if (splits < 1) splits = 1;
  const int m_per_split = ((mtiles + splits - 1) / splits) * 64;
  splits = (int)(((long)a.M + m_per_split - 1) / m_per_split);
  p.m_per_split = m_per_split; p.splits = splits; p.ny = ny;
  p.tp[0] = C;
  const long grid = 8L * ((splits + 7) / 8) * ny;                  // one token split (all its ny hidden blocks) per XCD
  // A DropPath factor that is uniform over every 64-token tile (none, or whole tiles per sample): the round-3 kernel.  Other sample lengths (96-px inputs, T = 20) take the
  // round-2 one, which looks the factor up per row and always adds with fp32 atomics.
  const bool tile_uniform = !a.row_scale || a.rows_per_scale % 64 == 0;
  if (!tile_uniform) {
    p.family = MVLT_MLP_WGRAD;
    p.block = NT;
    return bound(p, who, a.hid, wgrad_lds(C), grid);
  }
  const int nw = wgrad2_waves(C);
  p.family = MVLT_MLP_WGRAD2;
  p.tp[1] = nw;
  p.block = nw * 64;
  // the token splits' partial tiles of dW1 and dW2 as bf16 in the caller's scratch (ONE region for both) + two ordered folds behind the kernel, exactly where the fold
  // bookkeeping of gemm.hip hands out a region: a 16-byte aligned scratch that holds them and 16-byte aligned outputs.  Everything else: fp32 atomics, silently.
  p.partials_need = 2L * splits * a.hid * C * 2;
  p.fold = a.partials && aligned16(a.partials) && aligned16(a.dw1) && aligned16(a.dw2) && p.partials_need <= a.partials_bytes;
  if (p.fold) p.fold_grid[0] = p.fold_grid[1] = fold_wgs(a.hid, C);
  return bound(p, who, a.hid, wgrad2_lds(C, nw), grid);
}

}  // namespace mvlt_mlp

inline int plan_mlp_fwd(const mvlt_mlp_args& a, mvlt_mlp_plan& p) {
  using namespace mvlt_mlp;
  p = mvlt_mlp_plan{};
  if (int e = check(a, "mvlt_mlp_fwd")) return e;
  MVLT_REQUIRE(a.b2 && a.residual, "mvlt_mlp_fwd: b2 and residual are required");
  MVLT_REQUIRE(!a.out_op || aligned16(a.out_op), "mvlt_mlp_fwd: out_op must be 16-byte aligned");
  MVLT_REQUIRE(!a.post_y || (a.post_gamma && a.post_beta && a.post_mean && a.post_rstd && aligned16(a.post_y)),
               "mvlt_mlp_fwd: post_y needs post_gamma / post_beta / post_mean / post_rstd and 16-byte alignment");
  MVLT_REQUIRE(!a.ln_x || (a.ln_gamma && a.ln_beta && a.ln_y && a.ln_mean && a.ln_rstd && aligned16(a.ln_x) && aligned16(a.ln_y)),
               "mvlt_mlp_fwd: the folded LayerNorm needs gamma, beta, y, mean, rstd and 16-byte aligned rows");
  if (a.M <= 0) return MVLT_OK;                                    // MVLT_MLP_NONE
  return choose(a, 0, "mvlt_mlp_fwd", p);
}

inline int plan_mlp_bwd_dx(const mvlt_mlp_args& a, mvlt_mlp_plan& p) {
  using namespace mvlt_mlp;
  p = mvlt_mlp_plan{};
  if (int e = check(a, "mvlt_mlp_bwd_dx")) return e;
  MVLT_REQUIRE(a.dy && a.wc, "mvlt_mlp_bwd_dx: dy and wc (W2^T) are required");
  MVLT_REQUIRE(!a.lnb_x || (a.lnb_mean && a.lnb_rstd && a.lnb_gamma && a.lnb_dx && a.lnb_partials && (!a.lnb_dx2 || (a.lnb_dx2_scale && a.lnb_dx2_rows_per_scale > 0)) &&
                            aligned16(a.lnb_x) && aligned16(a.lnb_dx) && aligned16(a.lnb_dx2)),
               "mvlt_mlp_bwd_dx: lnb_x needs lnb_mean / lnb_rstd / lnb_gamma / lnb_dx / lnb_partials (and a scale for lnb_dx2), 16-byte aligned");
  if (a.M <= 0) return MVLT_OK;
  return choose(a, 1, "mvlt_mlp_bwd_dx", p);
}

inline int plan_mlp_bwd_dw(const mvlt_mlp_args& a, mvlt_mlp_plan& p) {
  using namespace mvlt_mlp;
  p = mvlt_mlp_plan{};
  MVLT_REQUIRE(a.x && a.dy && a.w1 && a.wc && a.b1 && a.dw1 && a.db1 && a.dw2 && a.db2, "mvlt_mlp_bwd_dw: null pointer");
  MVLT_REQUIRE(a.C == 64 || a.C == 128, "mvlt_mlp_bwd_dw: C must be 64 or 128, got %d", a.C);
  MVLT_REQUIRE(a.hid > 0 && a.hid % 128 == 0, "mvlt_mlp_bwd_dw: hidden size must be a multiple of 128");
  MVLT_REQUIRE(!a.row_scale || a.rows_per_scale > 0, "mvlt_mlp_bwd_dw: row_scale needs rows_per_scale");
  if (a.M <= 0) return MVLT_OK;
  return choose_dw(a, "mvlt_mlp_bwd_dw", p);
}

// the planned instantiation as mvlt_last_kernel() prints it ("" for MVLT_MLP_NONE); a change to a kernel's namespace or template parameters changes these literals
inline int plan_mlp_name(const mvlt_mlp_plan& p, char* buf, size_t n) {
  int w = -1;
  switch (p.family) {
    case MVLT_MLP_NONE: w = snprintf(buf, n, "%s", ""); break;
    case MVLT_MLP_FUSED: w = snprintf(buf, n, "mlp_fused_kernel<%d, %d>", p.tp[0], p.tp[1]); break;
    case MVLT_MLP_PIPE: w = snprintf(buf, n, "mlp_pipe_kernel<%d, %d>", p.tp[0], p.tp[1]); break;
    case MVLT_MLP_WGRAD: w = snprintf(buf, n, "mlp_wgrad_kernel<%d>", p.tp[0]); break;
    case MVLT_MLP_WGRAD2: w = snprintf(buf, n, "mlp_wgrad2_kernel<%d, %d>", p.tp[0], p.tp[1]); break;
    default: return -1;
  }
  return (w < 0 || (size_t)w >= n) ? -1 : w;
}

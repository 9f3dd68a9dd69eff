// Host side of the SR-attention entry points: argument checks, then the choice of kernel family, template arguments, launch geometry, dynamic LDS bytes and the two scalar
// kernel arguments -- a pure function of the argument struct (no HIP call, no global state, no launch; plain C++17, compiles with a host compiler alone).  attention.hip hands
// a plan to its family's file (attention_<family>.hip: one case list per family, no shape condition there); include/mvlt_hip_plan.h exports the plan, and
// tests/test_attn_plan_cpu.py pins it against launches recorded on an MI355X.  Every ladder of the dispatch is stated HERE, once; DESIGN.md ("Attention dispatch: plan, then
// launch") has the table of families.
#pragma once
#include <stdint.h>
#include <stdio.h>
#include "../../include/mvlt_hip_plan.h"
#include "plan_common.h"
#include "attention_common.h"

namespace mvlt_attn {

// the LDS-resident kernels take bf16 M <= 320 and fp32 M <= 288 (fp32 K / V^T of 320 keys: 164 864 B); the streamed ones everything beyond
inline bool resident(int M, int dtype) { return M <= (dtype == 0 ? 320 : 288); }
// round-3 forward (attn_fwd2_kernel, bf16) up to 192 keys (every 256-px configuration); beyond (272 keys at 384 px) its two score blocks no longer fit the
// register budget of two waves per SIMD next to the O accumulators (144 + 32 of 256), and the round-2 kernel is the faster one
constexpr int FWD2_MAX_M = 192;
// ... on four waves while two workgroups fit the 160 KB of a CU (up to 192 keys: 75.8 KB each), eight waves in ONE workgroup beyond (100 KB with four waves would
// leave one wave per SIMD; no such instantiation is reachable while FWD2_MAX_M is 192)
constexpr int fwd2_waves(int nkt) { return nkt <= 6 ? 4 : 8; }
constexpr int key_tiles(int M) { return (M + 31) / 32; }                // NKT: 32-key tiles
// resident backward: NW waves x TPW 16-key tiles per wave cover the padded keys
struct BwdRung { int max_m, nw, tpw; };
constexpr BwdRung BWD_LADDER[] = {{64, 4, 1}, {128, 4, 2}, {192, 4, 3}, {256, 8, 2}, {288, 6, 3}, {320, 8, 3}};
// workgroups the chip holds at once: two per CU for the four-wave bf16 instantiations, one otherwise
constexpr int bwd_slots(int dtype, int nw) { return (dtype == 0 && nw == 4) ? 512 : 256; }
inline int imin(int a, int b) { return a < b ? a : b; }
inline int imax(int a, int b) { return a > b ? a : b; }
inline long xcd_groups(long groups) { return 8 * ((groups + 7) / 8); }  // (batch, head) pairs in whole groups of the 8 XCDs

// Query chunks per (batch, head) of the backward.  With ONE chunk a workgroup sees every query of its (batch, head) and stores dK / dV plainly; every extra chunk
// adds M x 128 fp32 atomics per (batch, head) and pays the prologue (K^T staging, K / V fragments) again.  Round 1-5 took ceil(512 / groups) -- fill the chip once --
// which at pvlt_medium's stage 3 (320 (batch, head) pairs, 704 queries, 272 keys, one six-wave workgroup per CU) meant two chunks = 3 rounds of 11 query tiles + 22 M
// atomics: 175 us, where ONE chunk (2 rounds of 22 tiles, no atomics, no zero fill, no cast) takes 149 us (tools/ubench_attn.py sweep, profiles/r06_attn_bwd_chunks.txt).
// Round 6: the chunk count minimises a cost model fitted to that sweep and to the 256-px shapes -- rounds of the chip x (32-query tiles per chunk + 2 tiles of fixed
// cost) x 3.2 us, + chunks x groups x M x 128 atomics at 0.5 per ns when there is more than one chunk.  `slots` = workgroups the chip holds at once (two per CU for
// the four-wave bf16 instantiations, one otherwise).  It reproduces ceil(512 / groups) on every 256-px shape of the BASELINE configurations.
inline int bwd_chunks(int groups, int N, int M, int slots, bool one_chunk_only, int* q_per_wg) {
  int best_nq = 1;
  double best = -1.0;
  const int max_nq = one_chunk_only ? 1 : imin(128, imax(1, (N + 63) / 64));       // at least two query tiles per chunk
  for (int nq = 1; nq <= max_nq; ++nq) {
    const int qpw = ((N + nq - 1) / nq + 31) / 32 * 32;
    if ((N + qpw - 1) / qpw != nq) continue;                        // the rounding to whole tiles merged two chunks
    const long rounds = ((long)groups * nq + slots - 1) / slots;
    double cost = (double)rounds * (qpw / 32 + 2) * 3.2;
    if (nq > 1) cost += (double)nq * groups * M * 128.0 / 500.0 * 1e-3;
    if (best < 0.0 || cost < best) { best = cost; best_nq = nq; }
  }
  *q_per_wg = ((N + best_nq - 1) / best_nq + 31) / 32 * 32;
  return (N + *q_per_wg - 1) / *q_per_wg;
}

inline void set_plan(mvlt_attn_plan& p, int family, int block, size_t lds, int nq, int qpw, int t0, int t1 = 0, int t2 = 0) {
  p.family = family; p.block = block; p.lds = (int)lds; p.nq_chunks = nq; p.q_per_wg = qpw;
  p.tp[0] = t0; p.tp[1] = t1; p.tp[2] = t2; p.tp[3] = 0;
}

// The choice alone, for checked arguments (positive shape, dtype 0 / 1): everything of the plan but the grid, which comes back as a long for the caller to bound.
inline long choose_fwd(int B, int H, int N, int M, int dtype, bool streamed, mvlt_attn_plan& p) {
  const int es = dtype == 0 ? 2 : 4;
  const long groups = (long)B * H;
  if (streamed || !resident(M, dtype)) {                             // a workgroup is 4 waves x 32 queries
    const int kb = stream_kb_fwd(es);
    const long nq = (N + STREAM_QPW - 1) / STREAM_QPW;
    set_plan(p, MVLT_ATTN_FWD_STREAM, NT, fwd_stream_lds(es, kb), (int)nq, STREAM_QPW, dtype, kb);
    return xcd_groups(groups) * nq;
  }
  const int nkt = key_tiles(M);
  if (dtype == 0 && M <= FWD2_MAX_M) {
    const int nw = fwd2_waves(nkt);
    // a workgroup's waves walk its query chunk in 32-query tiles; chunks as long as the grid allows (K / V staging is per chunk):
    // at least ~1024 workgroups (two per CU, two rounds) when the problem has them
    int nq = 1;
    while (nq < 8 && (int)groups * nq < 1024 && (N + nq) / (nq + 1) >= 512) ++nq;
    const int qpw = ((N + nq - 1) / nq + 32 * nw - 1) / (32 * nw) * (32 * nw);
    nq = (N + qpw - 1) / qpw;
    set_plan(p, MVLT_ATTN_FWD2, nw * 64, fwd2_lds(nkt, nw), nq, qpw, nkt, M != nkt * 32, nw);
    return xcd_groups(groups) * nq;
  }
  int qpw = 256;
  if (N <= 512) qpw = 128 * ((N + 127) / 128);
  const int nq = (N + qpw - 1) / qpw;
  set_plan(p, MVLT_ATTN_FWD, NT, fwd_lds(es, nkt), nq, qpw, dtype, nkt);
  return xcd_groups(groups) * nq;
}

inline long choose_bwd(int B, int H, int N, int M, int dtype, bool one_chunk_only, bool streamed, mvlt_attn_plan& p) {
  const int es = dtype == 0 ? 2 : 4;
  const long groups = (long)B * H;
  if (streamed || !resident(M, dtype)) {                             // chunks of STREAM_QPW queries (the fp32 dQ tile the kernel keeps in LDS)
    const int nw = STREAM_BWD_NW, tpw = stream_bwd_tpw(es);
    const int qpw = imin(STREAM_QPW, (N + 31) / 32 * 32);
    const int nq = (N + qpw - 1) / qpw;
    set_plan(p, MVLT_ATTN_BWD_STREAM, nw * 64, bwd_stream_lds(es, nw, tpw), nq, qpw, dtype, nw, tpw);
    return xcd_groups(groups) * nq;
  }
  BwdRung r = BWD_LADDER[0];
  for (const BwdRung& x : BWD_LADDER) { r = x; if (M <= x.max_m) break; }
  int qpw = 0;
  const int nq = bwd_chunks((int)groups, N, M, bwd_slots(dtype, r.nw), one_chunk_only, &qpw);
  if (dtype == 0) set_plan(p, MVLT_ATTN_BWD_DMA, r.nw * 64, bwd_dma_lds(r.nw, r.tpw), nq, qpw, r.nw, r.tpw);
  else set_plan(p, MVLT_ATTN_BWD, r.nw * 64, bwd_lds(es, r.nw, r.tpw), nq, qpw, dtype, r.nw, r.tpw);
  return xcd_groups(groups) * nq;
}

}  // namespace mvlt_attn

inline int plan_attn_fwd(const mvlt_attn_args& a, bool force_streamed, mvlt_attn_plan& p) {
  using namespace mvlt_attn;
  const char* const fn = force_streamed ? "mvlt_sr_attention_fwd_streamed" : "mvlt_sr_attention_fwd";
  p = mvlt_attn_plan{};
  MVLT_REQUIRE(a.Q && a.KV && a.O, "%s: null pointer", fn);
  MVLT_REQUIRE(a.B > 0 && a.H > 0 && a.N > 0 && a.M > 0, "%s: bad shape", fn);
  MVLT_REQUIRE(a.dtype == 0 || a.dtype == 1, "%s: bad dtype", fn);
  const int pc = a.dtype == 0 ? 8 : 4;
  MVLT_REQUIRE(a.ldq % pc == 0 && a.ldkv % pc == 0 && a.ldo % pc == 0 && a.k_off % pc == 0 && a.v_off % pc == 0,
               "%s: strides/offsets must be multiples of %d elements", fn, pc);
  const long grid = choose_fwd(a.B, a.H, a.N, a.M, a.dtype, force_streamed, p);
  MVLT_REQUIRE(p.lds <= 160 * 1024, "mvlt_sr_attention_fwd: M=%d needs %zu B of LDS (>160 KB) in this dtype", a.M, (size_t)p.lds);
  MVLT_REQUIRE(grid <= 0x7fffffffL, "mvlt_sr_attention_fwd: %ld workgroups", grid);
  p.grid = (int)grid;
  return MVLT_OK;
}

inline int plan_attn_bwd(const mvlt_attn_bwd_args& a, bool force_streamed, mvlt_attn_plan& p) {
  using namespace mvlt_attn;
  const char* const fn = force_streamed ? "mvlt_sr_attention_bwd_streamed" : "mvlt_sr_attention_bwd";
  p = mvlt_attn_plan{};
  MVLT_REQUIRE(a.Q && a.KV && a.O && a.dO && a.lse && a.dQ && a.dKV, "%s: null pointer", fn);
  MVLT_REQUIRE(a.dkv_dtype == 1 || (a.dkv_dtype == 0 && a.dtype == 0),
               "%s: bf16 dKV needs bf16 operands (it forces one query chunk per (batch, head): plain stores)", fn);
  MVLT_REQUIRE(a.B > 0 && a.H > 0 && a.N > 0 && a.M > 0, "%s: bad shape", fn);
  MVLT_REQUIRE(a.dtype == 0 || a.dtype == 1, "%s: bad dtype", fn);
  const int pc = a.dtype == 0 ? 8 : 4;
  MVLT_REQUIRE(a.ldq % pc == 0 && a.ldkv % pc == 0 && a.ldo % pc == 0 && a.k_off % pc == 0 && a.v_off % pc == 0,
               "%s: strides/offsets must be multiples of %d elements", fn, pc);
  // a bf16 dKV is stored plainly, so it takes ONE query chunk: the resident kernels are given one, the streamed one (whose chunk is bounded by its LDS tile) refuses more
  const long grid = choose_bwd(a.B, a.H, a.N, a.M, a.dtype, a.dkv_dtype == 0, force_streamed, p);
  MVLT_REQUIRE(p.lds <= 160 * 1024, "mvlt_sr_attention_bwd: LDS %zu B > 160 KB", (size_t)p.lds);
  MVLT_REQUIRE(a.dkv_dtype == 1 || p.nq_chunks == 1,
               "mvlt_sr_attention_bwd: a bf16 dKV needs one query chunk per (batch, head); the streamed backward (M=%d) takes N <= %d for it, got N=%d",
               a.M, STREAM_QPW, a.N);
  MVLT_REQUIRE(grid <= 0x7fffffffL, "mvlt_sr_attention_bwd: %ld workgroups", grid);
  p.grid = (int)grid;
  return MVLT_OK;
}

// the planned instantiation as mvlt_last_kernel() prints it.  (The demangler does not know the bf16 type code DF16b: an instantiation over that element type keeps the
// runtime's mangled name, as gemm_plan.h's plan_kernel_name explains; a change to a kernel's namespace or signature changes these literals.)
inline int plan_attn_name(const mvlt_attn_plan& p, char* buf, size_t n) {
  const int* t = p.tp;
  const bool bf = t[0] == 0;
  int w = -1;
  switch (p.family) {
    case MVLT_ATTN_FWD:
      w = bf ? snprintf(buf, n, "_ZN12_GLOBAL__N_115attn_fwd_kernelIDF16bLi%dEEEv14mvlt_attn_argsii", t[1]) : snprintf(buf, n, "attn_fwd_kernel<float, %d>", t[1]);
      break;
    case MVLT_ATTN_FWD2: w = snprintf(buf, n, "attn_fwd2_kernel<%d, %s, %d>", t[0], t[1] ? "true" : "false", t[2]); break;
    case MVLT_ATTN_BWD:
      w = bf ? snprintf(buf, n, "_ZN12_GLOBAL__N_115attn_bwd_kernelIDF16bLi%dELi%dEEEv18mvlt_attn_bwd_argsii", t[1], t[2])
             : snprintf(buf, n, "attn_bwd_kernel<float, %d, %d>", t[1], t[2]);
      break;
    case MVLT_ATTN_BWD_DMA: w = snprintf(buf, n, "attn_bwd_dma_kernel<%d, %d>", t[0], t[1]); break;
    case MVLT_ATTN_FWD_STREAM:
      w = bf ? snprintf(buf, n, "_ZN12_GLOBAL__N_122attn_fwd_stream_kernelIDF16bLi%dEEEv14mvlt_attn_argsi", t[1]) : snprintf(buf, n, "attn_fwd_stream_kernel<float, %d>", t[1]);
      break;
    case MVLT_ATTN_BWD_STREAM:
      w = bf ? snprintf(buf, n, "_ZN12_GLOBAL__N_122attn_bwd_stream_kernelIDF16bLi%dELi%dEEEv18mvlt_attn_bwd_argsii", t[1], t[2])
             : snprintf(buf, n, "attn_bwd_stream_kernel<float, %d, %d>", t[1], t[2]);
      break;
    default: return -1;
  }
  return (w < 0 || (size_t)w >= n) ? -1 : w;
}

// Host side of mvlt_gemm_nt / mvlt_gemm_tn: argument checks, then the choice of kernel family, template arguments, launch geometry and trailing kernel
// arguments -- a pure function of the argument struct (no HIP call, no global state, no launch; plain C++17, compiles with a host compiler alone).
// gemm.hip hands a plan to its family's file (gemm_<family>.hip: one case list per family and entry point, no shape condition there); include/mvlt_hip_plan.h exports the plan, and
// tests/test_gemm_plan_cpu.py pins it against launches recorded on an MI355X.  The measured knowledge of the dispatch lives HERE; DESIGN.md ("GEMM dispatch: plan, then launch") has the table of families.
#pragma once
#include <stdint.h>
#include <stdio.h>
#include "../../include/mvlt_hip_plan.h"
#include "plan_common.h"        // MVLT_REQUIRE and the return codes where common.h is not there
#ifndef MVLT_NT_EARLY_DEFAULT
#define MVLT_NT_EARLY_DEFAULT 0x100  // early slot release in the NT K-loop: logits GEMM 172 -> 163 us, step -0.16 ms (same-box A/B, MVLT_NT_EARLY=0 / 1)
#endif

namespace mvlt_plan {

constexpr int BM = 128;               // rows of the 4-wave tiles
constexpr int NTHREADS = 256;
constexpr int ROW_BYTES = 128;        // one LDS row = 128 B of K
constexpr int TBK = 64;               // reduction rows per LDS tile of the TN kernels (both dtypes)
constexpr int TN_ROWB_BF16 = (TBK + 8) * 2, TN_ROWB_F32 = (TBK + 4) * 4;      // padded LDS rows of the register-staged TN kernel: 144 B / 272 B
constexpr int TN_TILE64_BYTES = TBK * 64 * 2;                                 // a 64-column bf16 tile of the LDS-DMA TN kernels
// (the kernels' own constants of these names and TElem<>::ROWB / DmaTile<64>::BYTES: gemm_common.h static_asserts that they agree)

inline bool al16(const void* p) { return ((uintptr_t)p & 15) == 0; }
inline int cdiv(int a, int b) { return (a + b - 1) / b; }
// workgroups of a launch whose leading grid factor is spread over the 8 XCDs (round-robin by workgroup id): whole groups of 8
inline int xcd_grid(int n) { return n >= 8 ? 8 * cdiv(n, 8) : n; }
inline int xcd_round(int splits) { return splits >= 8 ? (splits + 4) / 8 * 8 : splits; }

// ---- the split arithmetic of the TN kernels, once.  `ktiles` 64-row k-tiles are cut into m-splits: at most one split per k-tile, at least one; every split takes
// `per` k-tiles and the count is re-derived from that (the last split may be short, none is empty).
struct Split { int splits, per; };
inline Split split_even(int splits, int ktiles) {
  if (splits > ktiles) splits = ktiles;
  if (splits < 1) splits = 1;
  const int per = cdiv(ktiles, splits);
  return {cdiv(ktiles, per), per};
}
// ... for a launch that chooses: `want` splits fill the chip, each must bring min_tiles k-tiles of work to its flush, multiples of the 8 XCDs from 8 on.
// round_first: the 128-wide kernel rounds (and stops at 4096) BEFORE the work cap, so the cap's result is taken as it is (63 k-tiles: 7 splits; rounding after the
// cap would make 8 of them) -- the dgrad and the conv3x3 launches round after it.
inline Split split_choose(int want, int ktiles, int min_tiles, bool round_first) {
  if (round_first) { want = xcd_round(want); if (want > 4096) want = 4096; }
  if (want > ktiles / min_tiles) want = ktiles / min_tiles;
  if (!round_first) want = xcd_round(want);
  return split_even(want, ktiles);
}
inline int fold_workgroups(int N1, int N2) { return (int)(((long)N1 * N2 / 8 + 31) / 32); }
// the caller's scratch takes `need` bytes (the one fact mvlt_gemm_tn's fold bookkeeping can refuse on: null, misaligned or too small)
inline bool scratch_fits(const mvlt_gemm_tn_args& a, long need) { return a.partials && al16(a.partials) && need <= a.partials_bytes; }
inline void plan_fold(const mvlt_gemm_tn_args& a, mvlt_gemm_plan& p) {
  p.fold = 1;
  p.partials_need = (long)p.splits * a.N1 * a.N2 * 2;          // [splits][N1][N2] bf16
  p.fold_grid = fold_workgroups(a.N1, a.N2);
}

inline int check_rowmap(const mvlt_rowmap& m, const char* who) {
  if (m.mode == 0) {
    MVLT_REQUIRE(m.rows_per_batch >= 0, "%s: rows_per_batch < 0", who);
  } else if (m.mode == 1) {
    MVLT_REQUIRE(m.r > 0 && m.w_in > 0 && m.tokens_in > 0 && m.hw_out > 0 && m.w_out > 0 && m.c_seg > 0 && m.c_seg % 16 == 0,
                 "%s: bad patch map (c_seg must be a positive multiple of 16)", who);
  } else if (m.mode == 2) {
    MVLT_REQUIRE(m.r == 3 && m.w_in > 0 && m.h_in > 0 && m.tokens_in >= m.h_in * m.w_in && m.hw_out == m.h_in * m.w_in &&
                 m.w_out == m.w_in && m.c_seg > 0 && m.c_seg % 8 == 0, "%s: bad 3x3 neighbourhood map", who);
  } else {
    MVLT_REQUIRE(false, "%s: unknown rowmap mode %d", who, m.mode);
  }
  return MVLT_OK;
}

inline void set_tp(mvlt_gemm_plan& p, int family, int t0, int t1 = 0, int t2 = 0, int t3 = 0, int t4 = 0, int t5 = 0) {
  p.family = family;
  p.tp[0] = t0; p.tp[1] = t1; p.tp[2] = t2; p.tp[3] = t3; p.tp[4] = t4; p.tp[5] = t5;
}
inline void set_launch(mvlt_gemm_plan& p, int gx, int gy, int gz, int block, long lds) {
  p.grid[0] = gx; p.grid[1] = gy; p.grid[2] = gz; p.block = block; p.lds = (int)lds;
}
// the 8-wave / 8-phase NT kernel on a (64 HM) x (64 (HN0 + HN1)) tile: one workgroup per CU
inline void plan_nt_p8(const mvlt_gemm_nt_args& a, mvlt_gemm_plan& p, int epi, int hm, int hn0, int hn1, int rag) {
  const int bmt = 64 * hm, bnt = 64 * (hn0 + hn1);
  const int lds_loop = 2 * (2 * (2 * hm * 16) + 64 * (hn0 + hn1)) * 128, lds_epi = 8 * 32 * (16 * (hn0 + hn1) + 4) * 4;
  set_tp(p, MVLT_GEMM_NT_P8, epi, hm, hn0, hn1, rag);
  set_launch(p, 8 * cdiv(cdiv(a.M, bmt), 8) * cdiv(a.N, bnt), 1, 1, 512, lds_loop > lds_epi ? lds_loop : lds_epi);
}

}  // namespace mvlt_plan

inline int plan_gemm_nt(const mvlt_gemm_nt_args& a, mvlt_gemm_plan& p) {
  using namespace mvlt_plan;
  p = mvlt_gemm_plan{};
  MVLT_REQUIRE(a.A && a.B && a.C, "mvlt_gemm_nt: null operand");
  MVLT_REQUIRE(a.M >= 0 && a.N > 0 && a.K > 0, "mvlt_gemm_nt: bad shape M=%d N=%d K=%d", a.M, a.N, a.K);
  MVLT_REQUIRE(a.dtype == 0 || a.dtype == 1, "mvlt_gemm_nt: dtype must be 0 (bf16) or 1 (fp32)");
  const int pc = a.dtype == 0 ? 8 : 4;
  MVLT_REQUIRE(a.K % pc == 0 && a.lda % pc == 0 && a.ldb % pc == 0, "mvlt_gemm_nt: K/lda/ldb must be multiples of %d elements (16 B)", pc);
  MVLT_REQUIRE(al16(a.A) && al16(a.B), "mvlt_gemm_nt: A/B must be 16-byte aligned");
  MVLT_REQUIRE(a.act >= 0 && a.act <= 2, "mvlt_gemm_nt: bad act");
  MVLT_REQUIRE(a.act != 2 || a.H, "mvlt_gemm_nt: act=2 (gelu') needs H");
  MVLT_REQUIRE(!a.row_scale || a.rows_per_scale > 0, "mvlt_gemm_nt: row_scale needs rows_per_scale");
  MVLT_REQUIRE((a.col_sum == nullptr) == (a.col_sumsq == nullptr), "mvlt_gemm_nt: col_sum and col_sumsq come together");
  MVLT_REQUIRE(a.split_k <= 1 || (a.dtype == 0 && a.out_dtype == 1 && a.act == 0 && !a.H && !a.R && !a.row_scale && !a.col_sum &&
                                  a.c_map.mode == 0 && a.split_k <= 64),
               "mvlt_gemm_nt: split_k needs bf16 operands, fp32 C (zeroed by the caller) and a plain epilogue (A may be gathered)");
  MVLT_REQUIRE(a.col_copies >= 0, "mvlt_gemm_nt: col_copies < 0");
  MVLT_REQUIRE(!a.r_fp32 || (a.R && a.R != a.C && a.dtype == 0 && a.out_dtype == 0 && a.act == 0 && !a.col_sum && !a.post_y && a.split_k <= 1 && a.c_map.mode == 0 &&
                             a.N % 8 == 0 && a.ldc % 8 == 0 && (((uintptr_t)a.C | (uintptr_t)a.R) & 15) == 0 && a.M < (1 << 24)),
               "mvlt_gemm_nt: r_fp32 (fp32 residual beside a bf16 C) exists in the residual epilogue of the bf16 LDS-DMA kernels only (plain c_map, N % 8 == 0, 16-byte aligned C / R)");
  MVLT_REQUIRE(a.out_dtype >= 0 && a.out_dtype <= 2, "mvlt_gemm_nt: out_dtype is 0 (bf16), 1 (fp32) or 2 (fp16, with col_sum only)");
  MVLT_REQUIRE(a.out_dtype != 2 || (a.dtype == 0 && a.col_sum && a.act == 0 && !a.R && !a.row_scale && a.split_k <= 1 && a.c_map.mode == 0 && a.N % 8 == 0 &&
                                    a.ldc % 8 == 0 && al16(a.C) && a.M < (1 << 24)),
               "mvlt_gemm_nt: fp16 output exists in the column-statistics epilogue of the bf16 LDS-DMA kernels only (plain c_map, N % 8 == 0, 16-byte aligned C)");
  if (int e = check_rowmap(a.a_map, "mvlt_gemm_nt a_map")) return e;
  if (int e = check_rowmap(a.c_map, "mvlt_gemm_nt c_map")) return e;
  MVLT_REQUIRE(a.a_map.mode == 0 || a.K == a.a_map.r * a.a_map.r * a.a_map.c_seg, "mvlt_gemm_nt: gather K != r*r*c_seg");
  MVLT_REQUIRE(a.c_map.mode == 0 || a.N == a.c_map.r * a.c_map.r * a.c_map.c_seg, "mvlt_gemm_nt: scatter N != r*r*c_seg");
  MVLT_REQUIRE(a.c_map.mode != 2, "mvlt_gemm_nt: the 3x3 map is a gather only (its dgrad is a gather with flipped taps)");
  // EPI 8 (LayerNorm of the finished row) exists in the bf16 LDS-DMA kernel only: every other launch path refuses instead of skipping it silently
  MVLT_REQUIRE(!a.post_y || (a.dtype == 0 && a.split_k <= 1),
               "mvlt_gemm_nt: post_y needs the bf16 LDS-DMA path (no fp32 operands, no split_k)");
  if (a.M == 0) return MVLT_OK;
  const int tiles_m = cdiv(a.M, BM);
  const bool narrow = a.N <= 64;
  const int bn = narrow ? 64 : 128;
  const int tiles_n = cdiv(a.N, bn);
  const int ksplit = a.split_k > 1 ? a.split_k : 1;
  const long stage = (long)4 * 32 * (bn / 2 + 4) * sizeof(float);      // epilogue staging (4 waves x 32 rows)
  const int gx = 8 * cdiv(tiles_m, 8) * tiles_n;                        // m-tiles in whole groups of the 8 XCDs
  if (a.dtype != 0) {                                                  // fp32 operands: the exact-f32 kernel, register-staged
    p.nbuf = a.K <= 32 ? 1 : 2;
    const long lds = (long)p.nbuf * (BM + bn) * ROW_BYTES;
    set_tp(p, MVLT_GEMM_NT_F32, bn);
    set_launch(p, gx, ksplit, 1, NTHREADS, lds < stage ? stage : lds);
    return MVLT_OK;
  }
  // compile-time epilogue variant (see nt_epilogue_lean); 0 = generic
  int epi = 0;
  // (N % 8 != 0 -- the 30522-word MLM logits -- takes the plain lean epilogue too: its last chunk of a row is stored column by column)
  const bool plain_epi = a.act == 0 && !a.R && !a.row_scale && !a.col_sum && !a.H && a.c_map.mode == 0;
  const bool lean_ok = (a.c_map.mode == 0 || (a.c_map.mode == 1 && a.c_map.c_seg % 8 == 0)) && a.split_k <= 1 && (a.N % 8 == 0 || plain_epi) && a.ldc % 8 == 0 && al16(a.C) &&
                       (!a.R || al16(a.R)) && (!a.H || al16(a.H)) && a.M < (1 << 24);
  if (lean_ok && a.c_map.mode == 1) {
    if (a.act == 0 && !a.col_sum && !a.R && !a.row_scale) epi = 6;
    else if (a.act == 0 && !a.col_sum && a.R) epi = 7;
  } else if (lean_ok) {
    if (a.act == 1 && !a.R && !a.row_scale && !a.col_sum && a.out_dtype == 0) epi = 3;
    else if (a.act == 2 && !a.R && !a.row_scale && !a.col_sum && a.out_dtype == 0) epi = 4;
    else if (a.act == 0 && a.R && !a.col_sum) epi = 2;
    else if (a.act == 0 && !a.R && !a.row_scale && a.col_sum) epi = 5;
    else if (a.act == 0 && !a.R && !a.row_scale && !a.col_sum) epi = 1;
  }
  // ring depth: 2 stages (64 KB, two workgroups per CU).  A single stage at four workgroups per CU was tried: same time in
  // the step, and its extra in-loop issue path cost 34 VGPRs (a wave per SIMD on the K <= 64 launches)
  // The GELU epilogue (EPI 3) on the short-K fc1 GEMMs is epilogue-bound: 32-wide K stages halve the ring (32 KB) so a third
  // workgroup fits per CU and covers it (98304x1280x320: 240 -> 220 us, 49152x2048x512: 234 -> 201 us).  Long K loses to the
  // doubled barrier count (K = 2048: 103 -> 125 us), other epilogues are neutral; EPI 4 prefers its two-half H prefetch,
  // whose registers allow two workgroups per CU either way (220 / 213 us against 227 / 217 us).
  const int bk = (!narrow && a.a_map.mode == 0 && (epi == 3 || epi == 4) && a.K <= 512) ? 32 : 64;
  const int nk = bk == 32 ? cdiv(a.K, 32) : cdiv(cdiv(a.K, 64), ksplit);
  const int ns = nk < 2 ? nk : 2;
  p.ns_flags = nk >= 2 ? ns | MVLT_NT_EARLY_DEFAULT : ns;               // (a single k-step has nothing to refill)
  long lds = (long)ns * (BM + bn) * (bk * 2);
  if (lds < stage) lds = stage;
  if (a.post_y) {                            // EPI 8: attn.proj + residual + Block.norm2 (whole rows in one tile)
    MVLT_REQUIRE(epi == 2 && a.N == bn && a.a_map.mode == 0 && a.c_map.mode == 0 && a.c_map.rows_per_batch == 0 && a.post_gamma && a.post_beta &&
                 a.post_mean && a.post_rstd && a.post_ld % 8 == 0 && al16(a.post_y) && al16(a.post_gamma),
                 "mvlt_gemm_nt: post_y needs bf16 operands, a residual (R), N == 64 or 128, identity row maps, 16-byte aligned outputs");
    set_tp(p, MVLT_GEMM_NT_DMA, bn, 0, 8, 64);
    set_launch(p, gx, ksplit, 1, NTHREADS, lds < stage + 2048 ? stage + 2048 : lds);
    return MVLT_OK;
  }
  // conv3x3 (a_map mode 2) on an LDS-resident, channel-sliced halo: grids of width 16 / 32 / 64, whole 128-pixel tiles inside one
  // image, 64-multiples of gathered channels, lean epilogue, identity or batch-strided output rows
  if (a.a_map.mode == 2 && (epi == 1 || epi == 2 || epi == 5) && a.split_k <= 1 && a.a_map.c_seg % 64 == 0 && a.c_map.mode == 0 &&
      (a.a_map.w_in == 16 || a.a_map.w_in == 32 || a.a_map.w_in == 64) && (a.a_map.h_in * a.a_map.w_in) % BM == 0 && a.M % BM == 0 &&
      a.M % (a.a_map.h_in * a.a_map.w_in) == 0 && a.a_map.hw_out == a.a_map.h_in * a.a_map.w_in && a.a_map.w_out == a.a_map.w_in &&
      a.K == 9 * a.a_map.c_seg && a.lda >= a.a_map.c_seg && a.ldb >= a.K) {
    const int w = a.a_map.w_in;
    // N % 192 == 0 (the 192-channel convolutions): one 192-wide tile instead of 128 + a half-empty 128 (statistics / plain epilogue only)
    const int cbn = (a.N % 192 == 0 && a.N % 128 != 0 && epi != 2) ? 192 : a.N <= 64 ? 64 : 128;
    const int halo_rows = (BM / w + 2) * (w + 2), h_it = cdiv(halo_rows * 8, NTHREADS);
    const long clds = (long)h_it * NTHREADS * 16 + (long)2 * cbn * ROW_BYTES, cstage = (long)4 * 32 * (cbn / 2 + 4) * sizeof(float);
    set_tp(p, MVLT_GEMM_NT_CONV3, w, cbn, epi);
    set_launch(p, 8 * cdiv(a.M / BM, 8) * cdiv(a.N, cbn), 1, 1, NTHREADS, clds < cstage ? cstage : clds);
    return MVLT_OK;
  }
  // 8-wave kernels with the 8-phase K-loop (gemm_nt_p8_kernel) for the MFMA-bound shapes of the stage 3-4 MLPs: one workgroup per CU, so the
  // tile height is chosen by whole rounds of 256 CUs (rows x rounds = time): 256 x 256, 192 x 256, or 192 x 320 for N % 320 == 0
  if (a.a_map.mode == 0 && a.a_map.rows_per_batch == 0 && a.c_map.mode == 0 && epi >= 1 && epi <= 5 && a.K % 64 == 0 && a.K >= 128) {
    auto cost = [&](int bm, int bnt) -> long {                         // rows x rounds; 0 = shape does not fit
      if (a.M % bm || a.N % bnt) return 0;
      const long tiles = (long)(a.M / bm) * (a.N / bnt);
      if (tiles < 192) return 0;
      return ((tiles + 255) / 256) * (long)bm * bnt;
    };
    // a ragged last tile pays when the whole rounds of padded tiles are at least 85 % real work
    auto mostly_real = [&](long tiles, double tile_elems) { return (double)a.M * a.N >= 0.85 * (double)((tiles + 255) / 256) * 256.0 * tile_elems; };
    const long c256 = cost(256, 256), c192 = cost(192, 256);
    // (192 x 320 with the fp32 residual epilogue pays from K = 640 on: 98304 x 320 x 320 + R 93 us against 73 us on the 128-wide kernel, K = 1280 138 against 155;
    //  the 320-wide tile has the plain and the residual epilogue only)
    const bool epi320 = a.N % 256 != 0 && (epi == 1 || (epi == 2 && a.K >= 640));
    const long c320 = epi320 ? cost(192, 320) : 0;
    if (!c320 && !c256 && !c192) {
      // ragged M / N (the MLM logits, ~1500 x 30522 x 768, fp32 out): 256 x 256 tiles with the loader clamped at the last row and the checked epilogue:
      // 294912 x 128 would pad half of every 256-wide tile (36 -> 56 us), and 1558 selected rows make 7 x 120 tiles = 4 rounds where 1490 rows make 3
      // (the 128-wide kernel then wins)
      const long t256 = (long)cdiv(a.M, 256) * cdiv(a.N, 256);
      if (epi == 1 && (a.M % 256 || a.N % 256) && t256 >= 384 && mostly_real(t256, 65536.0)) { plan_nt_p8(a, p, 1, 4, 2, 2, 1); return MVLT_OK; }
      // ragged M on the 192 x 320 tile (N % 320 == 0, same epilogue rules as the whole-tile form): pvlt_medium at 384 px runs its 18 stage-3 blocks at
      // M = 45056 = 234.67 x 192 rows -- 235 tiles = ONE round at 92 % -- and took the 128-wide kernels for every N = 320 product (fc2 76 us, fc1 input
      // gradient 66 us, q / proj 27 us: profiles/r06_medium384_gemm_shapes.txt)
      const long t320 = (long)cdiv(a.M, 192) * (a.N / 320);
      if (epi320 && a.N % 320 == 0 && a.M % 192 != 0 && t320 >= 192 && mostly_real(t320, 192.0 * 320.0)) { plan_nt_p8(a, p, epi, 3, 3, 2, 1); return MVLT_OK; }
    }
    if (c320) { plan_nt_p8(a, p, epi, 3, 3, 2, 0); return MVLT_OK; }
    if (c256 && (!c192 || c256 <= c192)) { plan_nt_p8(a, p, epi, 4, 2, 2, 0); return MVLT_OK; }
    if (c192) { plan_nt_p8(a, p, epi, 3, 2, 2, 0); return MVLT_OK; }
  }
  // N % 192 == 0 (the 192-channel convolutions): one 192-wide tile instead of 128 + a half-empty 128
  if (!narrow && a.N % 192 == 0 && a.N % 128 != 0 && (epi == 1 || epi == 5) && a.c_map.mode == 0 && a.a_map.mode != 1 && a.K >= 128) {
    const long lds192 = (long)ns * (BM + 192) * ROW_BYTES, stage192 = (long)4 * 32 * 100 * sizeof(float);
    set_tp(p, MVLT_GEMM_NT_DMA, 192, a.a_map.mode, epi, 64);
    set_launch(p, 8 * cdiv(tiles_m, 8) * (a.N / 192), 1, 1, NTHREADS, lds192 < stage192 ? stage192 : lds192);
    return MVLT_OK;
  }
  set_tp(p, MVLT_GEMM_NT_DMA, bn, a.a_map.mode, epi, bk);
  set_launch(p, gx, ksplit, 1, NTHREADS, lds);
  return MVLT_OK;
}

inline int plan_gemm_tn(const mvlt_gemm_tn_args& a, mvlt_gemm_plan& p) {
  using namespace mvlt_plan;
  p = mvlt_gemm_plan{};
  MVLT_REQUIRE(a.A && a.B && a.C, "mvlt_gemm_tn: null operand");
  MVLT_REQUIRE(a.M >= 0 && a.N1 > 0 && a.N2 > 0, "mvlt_gemm_tn: bad shape");
  MVLT_REQUIRE(a.dtype == 0 || a.dtype == 1, "mvlt_gemm_tn: dtype must be 0 (bf16) or 1 (fp32)");
  const int pc = a.dtype == 0 ? 8 : 4;
  // N1/N2 may be ragged (30522 vocabulary rows) as long as the padded row (lda/ldb) covers the last 16-B chunk
  MVLT_REQUIRE(a.lda % pc == 0 && a.ldb % pc == 0, "mvlt_gemm_tn: lda/ldb must be multiples of %d elements (16 B)", pc);
  MVLT_REQUIRE(a.lda >= (a.N1 + pc - 1) / pc * pc, "mvlt_gemm_tn: lda must cover N1 rounded up to %d", pc);
  MVLT_REQUIRE(a.b_map.mode != 0 || a.ldb >= (a.N2 + pc - 1) / pc * pc, "mvlt_gemm_tn: ldb must cover N2 rounded up to %d", pc);
  MVLT_REQUIRE(al16(a.A) && al16(a.B), "mvlt_gemm_tn: A/B must be 16-byte aligned");
  if (int e = check_rowmap(a.a_map, "mvlt_gemm_tn a_map")) return e;
  if (int e = check_rowmap(a.b_map, "mvlt_gemm_tn b_map")) return e;
  MVLT_REQUIRE(a.a_map.mode == 0, "mvlt_gemm_tn: A cannot be a patch gather");
  MVLT_REQUIRE(!(a.colsum_a && a.colsum_b), "mvlt_gemm_tn: at most one of colsum_a / colsum_b");
  MVLT_REQUIRE(a.b_map.mode == 0 || a.N2 == a.b_map.r * a.b_map.r * a.b_map.c_seg, "mvlt_gemm_tn: gather N2 != r*r*c_seg");
  MVLT_REQUIRE(a.c_taps <= 1 || (a.trans_c == 0 && a.c_seg > 0 && a.N2 == a.c_taps * a.c_seg), "mvlt_gemm_tn: c_taps needs trans_c == 0 and N2 == c_taps*c_seg");
  MVLT_REQUIRE(!a.dgrad_out || (a.dtype == 0 && a.M < (1 << 24) && a.b_map.mode == 0 && a.a_map.mode == 0),
               "mvlt_gemm_tn: dgrad_out rides on the bf16 LDS-DMA kernel only (bf16 operands, M < 2^24, plain row maps): every other path would leave it unwritten");
  if (a.M == 0) return MVLT_OK;
  const int mtiles = cdiv(a.M, TBK);
  // a split of the LDS-DMA kernel must bring at least 8 k-tiles of work to its N1*N2 atomics: the kv / text-row weight gradients (32768 or 16384
  // rows, 256 x 128 outputs) ran 256 splits of 1-2 k-tiles, 49 us where 32-64 splits take 20-26 us
  constexpr int TN_MIN_TILES = 8;
  // conv3x3 weight gradient with an LDS-resident halo (conv3_wgrad_kernel): 3x3 gather on B over a W x H grid with W in {8, 16, 32, 64},
  // whole 64-pixel k-tiles inside one image, 64-multiples of channels, plain [out][tap*cin + c] output
  if (a.dtype == 0 && a.b_map.mode == 2 && a.a_map.mode == 0 && a.a_map.rows_per_batch == 0 && !a.trans_c && a.c_taps <= 1 &&
      !a.colsum_a && !a.colsum_b && a.N1 % 64 == 0 && a.b_map.c_seg % 64 == 0 && a.N2 == 9 * a.b_map.c_seg && a.M % 64 == 0 &&
      (a.b_map.w_in == 8 || a.b_map.w_in == 16 || a.b_map.w_in == 32 || a.b_map.w_in == 64) && (a.b_map.h_in * a.b_map.w_in) % 64 == 0 &&
      a.M % (a.b_map.h_in * a.b_map.w_in) == 0 && a.ldb >= a.b_map.c_seg) {
    const int w = a.b_map.w_in, halo_rows = (64 / w + 2) * (w + 2), h_it = cdiv(halo_rows * 8, NTHREADS);
    const long lds = (long)2 * (TN_TILE64_BYTES + h_it * NTHREADS * 16);                   // two stages of a 64 x 64 bf16 tile + the halo
    const int n_o = a.N1 / 64, n_c = a.b_map.c_seg / 64;
    // every split flushes its whole 64 x 576 block with fp32 atomics: at least 16 k-tiles of work per flush, about two workgroups per
    // CU when the shape allows (262144 x 64 x 576: 640 splits of 7 tiles 108 us, 256 splits of 16 tiles measured below)
    const Split sp = split_choose(cdiv(512, n_o * n_c), a.M / 64, 16, false);
    set_tp(p, MVLT_GEMM_TN_CONV3, w);
    set_launch(p, xcd_grid(sp.splits) * n_o * n_c, 1, 1, NTHREADS, lds);
    p.per_split = sp.per; p.t1 = n_o; p.t2 = n_c; p.splits = sp.splits;
    // from 4 splits on the caller's scratch takes the splits' blocks (bf16) and an ordered fold adds them to C: no atomics (the blocks are staged in the loop's LDS)
    if (sp.splits >= 4 && a.ldc % 4 == 0 && al16(a.C) && lds >= (long)4 * 16 * (9 * 32 + 8) * 2 && scratch_fits(a, (long)sp.splits * a.N1 * a.N2 * 2)) plan_fold(a, p);
    return MVLT_OK;
  }
  // (Round 4 built this kernel's 8-wave / 8-phase sibling -- 256 x 256 and 128 x 320 output tiles, one workgroup per CU, commit 6d0e8d3 -- and
  //  removed it again: its main loop ran at 1.1-1.16 PFLOP/s, but one workgroup per CU means 16 m-splits of the 2048 x 512 outputs, and the fp32
  //  atomics that combine the splits complete at ~0.3 floats per ns chip-wide whatever their scope or coalescing: 55 us of tail per launch,
  //  147 us against the 122 us of the 128 x 128 tiles below with their 8 splits and a second workgroup per CU to hide the tail.  DESIGN.md 6.)
  // The 8-wave / 8-phase TN loop (gemm_tn_p8_kernel) with bf16 partial tiles + an ordered fold instead of fp32 atomics: plain rows, a scratch from the caller
  if (a.partials && a.dtype == 0 && a.a_map.mode == 0 && a.b_map.mode == 0 && a.a_map.rows_per_batch == 0 && a.b_map.rows_per_batch == 0 && a.c_taps <= 1 &&
      !a.trans_c && !a.dgrad_out && a.M % 64 == 0 && a.ldc % 4 == 0 && al16(a.C) && al16(a.partials)) {
    const int nkt = a.M / 64;
    // whole 256 x 256 output tiles, 16 .. 64 of them (= 16 .. 4 m-splits for one workgroup per CU).  Fewer tiles mean more splits than the fold is
    // worth (8 tiles: 75 us either way), more do not occur in this model.
    if (a.N1 % 256 == 0 && a.N2 % 256 == 0) {
      const int t1 = a.N1 / 256, t2 = a.N2 / 256, tiles = t1 * t2;
      if (tiles >= 16 && tiles <= 64 && nkt / (256 / tiles) >= 16 && a.partials_bytes >= (long)(256 / tiles) * a.N1 * a.N2 * 2) {
        const Split sp = split_even(256 / tiles, nkt);                 // one workgroup per CU (the caller's scratch is sized for exactly this)
        set_tp(p, MVLT_GEMM_TN_P8, 4, 2, 2, 1, 0, 0);
        set_launch(p, xcd_grid(sp.splits) * tiles, 1, 1, 512, 2 * 64 * 2 * (2 * (2 * 4 * 16) + 256));
        p.per_split = sp.per; p.t1 = t1; p.t2 = t2; p.splits = sp.splits;
        plan_fold(a, p);
        return MVLT_OK;
      }
    }
    // round 6: one side a multiple of 320, the other >= 1024 (the fc weight gradients of stage 3: 1280 x 320 and 320 x 1280): 192 x 320 tiles of the 8-phase TN loop, 6-16 of
    // them, the last row tile ragged when it is >= 85 % full overall (round 5 ran them on the 128-wide kernel).  swapped: the 320 side is the caller's N1 -- the kernel
    // gets the operands exchanged and stores its partial tiles transposed, i.e. in the caller's layout
    const bool direct = a.N2 % 320 == 0 && a.N1 >= 1024, swapped = !direct && a.N1 % 320 == 0 && a.N2 >= 1024;
    if ((direct || swapped) && a.N1 % 8 == 0 && a.N2 % 8 == 0 && a.lda % 8 == 0 && a.ldb % 8 == 0) {
      const int rows = direct ? a.N1 : a.N2, cols = direct ? a.N2 : a.N1;
      const int t1 = cdiv(rows, 192), t2 = cols / 320, tiles = t1 * t2;
      if (tiles >= 6 && tiles <= 16 && nkt / (256 / tiles) >= 16 && (double)rows >= 0.85 * 192.0 * t1) {
        // all tiles of an m-split run on ONE XCD (32 CUs, one workgroup each): whole splits per XCD, the same number on each -- 7 tiles: 4 splits per XCD = 32 splits = 224
        // workgroups (36 splits = 252 workgroups put 35 on four of the XCDs: a second round there, 184 us instead of the 128-wide kernel's 137)
        const Split sp = split_even((32 / tiles) * 8 >= 8 ? (32 / tiles) * 8 : 256 / tiles, nkt);
        if (scratch_fits(a, (long)sp.splits * a.N1 * a.N2 * 2)) {      // (does not fit: the 128-wide kernel below)
          set_tp(p, MVLT_GEMM_TN_P8, 3, 3, 2, direct, rows % 192 != 0, swapped);
          set_launch(p, xcd_grid(sp.splits) * tiles, 1, 1, 512, 2 * 64 * 2 * (2 * (2 * 3 * 16) + 320));
          p.per_split = sp.per; p.t1 = t1; p.t2 = t2; p.splits = sp.splits; p.swap_operands = swapped;
          plan_fold(a, p);
          return MVLT_OK;
        }
      }
    }
  }
  if (a.dtype == 0 && a.M < (1 << 24)) {
    // LDS-DMA kernel: A tile 128 or 64 wide, B tile 128 or 64 wide; ~1024 workgroups, splits a multiple of the 8 XCDs
    if (a.dgrad_out) {
      // weight gradient + input gradient of a C x C Linear from one pass over dY (gemm_tn_dma_kernel<.., DG>): one output tile, plain rows
      MVLT_REQUIRE(a.dgrad_wt && a.N1 == a.N2 && (a.N1 == 64 || a.N1 == 128) && a.a_map.rows_per_batch == 0 && a.b_map.mode == 0 &&
                   a.b_map.rows_per_batch == 0 && !a.trans_c && a.c_taps <= 1 && !a.colsum_b && a.dgrad_ld % 8 == 0 &&
                   (((uintptr_t)a.dgrad_out | (uintptr_t)a.dgrad_wt) & 15) == 0,
                   "mvlt_gemm_tn: dgrad_out needs bf16 operands, plain rows, N1 == N2 == 64 or 128, no transposed / tap output, 16-byte aligned buffers");
      // 1081344 x 64: 128 / 192 / 256 / 384 / 512 splits 136 / 90 / 83 / 91 / 85 us; 294912 x 128: 75 / 63 / 60 / 59 / 68
      const Split sp = split_choose(a.splits > 0 ? a.splits : (a.N1 == 64 ? 256 : 384), mtiles, TN_MIN_TILES, false);
      const int ns = a.N1 == 64 ? 4 : 2;
      set_tp(p, MVLT_GEMM_TN_DMA, a.N1, a.N1, 3, ns, 1);
      set_launch(p, xcd_grid(sp.splits), 1, 1, NTHREADS, (long)ns * TBK * 2 * a.N1 * 2 + 64 * a.N1 * 2);      // the ring + the W^T tile
      p.per_split = sp.per * TBK; p.t1 = 1; p.t2 = 1; p.splits = sp.splits;
      return MVLT_OK;
    }
    MVLT_REQUIRE(!a.c_overwrite || (!a.trans_c && a.c_taps <= 1 && a.N2 % 4 == 0 && a.ldc % 4 == 0 && al16(a.C)),
                 "mvlt_gemm_tn: c_overwrite needs the plain output layout, N2 % 4 == 0, ldc % 4 == 0 and a 16-byte aligned C");
    // outputs of at most 128 x 128 take 64 x 64 tiles: every output cache line receives one atomic request per m-split, those
    // serialise at the memory side (~100 ns each), and four small tiles need a quarter of the splits of one big tile for the same
    // number of workgroups (294912 x 128 x 128: 61 -> 35 us)
    const bool small_out = a.N1 <= 128 && a.N2 <= 128;
    const int bmt = (a.N1 <= 64 || small_out) ? 64 : 128, bn = (a.N2 <= 64 || small_out) ? 64 : 128;
    const int t1 = cdiv(a.N1, bmt), t2 = cdiv(a.N2, bn);
    // 2 workgroups per CU in one round: every extra split is another N1*N2 fp32 atomics through the fabric; a single output tile: 384 (1081344 x 64 x 64: 54.7 -> 48.9 us)
    const int given = a.c_overwrite ? 1 : a.splits;
    const Split sp = given > 0 ? split_even(given, mtiles) : split_choose(cdiv(t1 * t2 == 1 ? 384 : 512, t1 * t2), mtiles, TN_MIN_TILES, true);
    const int ns = (bmt + bn == 256) ? 2 : (bmt + bn == 192) ? 3 : 4;      // 64 / 72 / 64 KB of LDS: 2 workgroups per CU
    const int bmode = (a.b_map.mode == 0 && a.b_map.rows_per_batch == 0 && a.a_map.rows_per_batch == 0) ? 3 : a.b_map.mode;      // 3: plain rows on both operands
    set_tp(p, MVLT_GEMM_TN_DMA, bmt, bn, bmode, ns, 0);
    set_launch(p, xcd_grid(sp.splits) * t1 * t2, 1, 1, NTHREADS, (long)ns * TBK * (bmt + bn) * 2);
    p.per_split = sp.per * TBK; p.t1 = t1; p.t2 = t2; p.splits = sp.splits;
    // several splits meeting on an output of >= 65536 elements (>= 8: the C x C and the fc weight gradients of stages 3-4; 24 while every fold was a launch of its own -- with the
    // batched folds 16 / 8 / 4 / 2 all measure 12.98-13.00 k pairs/s against 12.90 at 24): bf16 partial tiles into the caller's scratch
    // + an ordered fold instead of the atomics (14-21 us of a 53-56 us launch, profiles/r05_tn_small_atomics_ablation.txt).  Fewer splits: the atomics are cheaper than a fold launch.
    constexpr int part_min = 8;
    // ... and from 16384 output elements on (65536 through round 5): the SMALL outputs are where many splits hurt most -- text_embed1's 64 x 768 weight gradient over 32768 rows:
    // 64 splits x 49152 atomics on the same 1536 cache lines = 56 us where its operands are 9 us of HBM time (tools/ubench_tn_smallk.py)
    constexpr long part_min_out = 16384;
    if (!a.c_overwrite && sp.splits >= part_min && !a.trans_c && a.c_taps <= 1 && a.N2 % 8 == 0 && a.ldc % 4 == 0 && al16(a.C) && (long)a.N1 * a.N2 >= part_min_out &&
        scratch_fits(a, (long)sp.splits * a.N1 * a.N2 * 2))
      plan_fold(a, p);
    return MVLT_OK;
  }
  // fp32 operands (and bf16 past 2^24 rows): the register-staged kernel, ~4 workgroups per CU in total, fp32 atomics
  const int bn = a.N2 <= 64 ? 64 : 128;
  const int t1 = cdiv(a.N1, BM), t2 = cdiv(a.N2, bn);
  const int want = cdiv(1024, t1 * t2);
  const Split sp = split_even(a.splits > 0 ? a.splits : (want > 4096 ? 4096 : want), mtiles);
  const int rowb = a.dtype == 0 ? TN_ROWB_BF16 : TN_ROWB_F32;
  set_tp(p, MVLT_GEMM_TN_PLAIN, a.dtype, bn);
  set_launch(p, t1, t2, sp.splits, NTHREADS, (long)(BM + bn) * rowb + BM * sizeof(float));
  p.per_split = sp.per * TBK; p.splits = sp.splits;
  return MVLT_OK;
}

// the planned instantiation as the demangler prints it (template arguments separated by ", ", bool as true / false)
inline int plan_kernel_name(const mvlt_gemm_plan& p, char* buf, size_t n) {
  const int* t = p.tp;
  const char* tf[2] = {"false", "true"};
  int w = -1;
  switch (p.family) {
    case MVLT_GEMM_NONE: w = snprintf(buf, n, "%s", ""); break;
    case MVLT_GEMM_NT_F32: w = snprintf(buf, n, "gemm_nt_kernel<float, %d>", t[0]); break;
    case MVLT_GEMM_NT_DMA: w = snprintf(buf, n, "gemm_nt_dma_kernel<%d, %d, %d, %d, 128>", t[0], t[1], t[2], t[3]); break;
    case MVLT_GEMM_NT_P8: w = snprintf(buf, n, "gemm_nt_p8_kernel<%d, %d, %d, %d, %s>", t[0], t[1], t[2], t[3], tf[t[4] != 0]); break;
    case MVLT_GEMM_NT_CONV3: w = snprintf(buf, n, "conv3_nt_kernel<%d, %d, %d>", t[0], t[1], t[2]); break;
    case MVLT_GEMM_TN_PLAIN:        // (the demangler does not know the bf16 type code DF16b: mvlt_last_kernel() hands out that name as the runtime has it, mangled.
                                    //  A toolchain that demangles it, or a change to the kernel's namespace or signature, changes what mvlt_last_kernel() prints: this
                                    //  literal then has to follow -- tests/test_exact_gpu.py::test_gemm_tn_bf16_past_2_24_rows launches it, the fixture holds its name)
      w = t[0] == 0 ? snprintf(buf, n, "_ZN12_GLOBAL__N_114gemm_tn_kernelIDF16bLi%dEEEv17mvlt_gemm_tn_argsi", t[1]) : snprintf(buf, n, "gemm_tn_kernel<float, %d>", t[1]);
      break;
    case MVLT_GEMM_TN_DMA: w = snprintf(buf, n, "gemm_tn_dma_kernel<%d, %d, %d, %d, %s>", t[0], t[1], t[2], t[3], tf[t[4] != 0]); break;
    case MVLT_GEMM_TN_P8: w = snprintf(buf, n, "gemm_tn_p8_kernel<%d, %d, %d, %s, %s, %s>", t[0], t[1], t[2], tf[t[3] != 0], tf[t[4] != 0], tf[t[5] != 0]); break;
    case MVLT_GEMM_TN_CONV3: w = snprintf(buf, n, "conv3_wgrad_kernel<%d>", t[0]); break;
    default: return -1;
  }
  return (w < 0 || (size_t)w >= n) ? -1 : w;
}

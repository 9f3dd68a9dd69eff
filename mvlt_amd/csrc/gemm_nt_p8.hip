// NT GEMM, bf16, 8 waves, 8-phase K-loop (256 x 256 x 64 and relatives).  Overview: gemm.hip.
#include "gemm_common.h"

namespace {

// ------------------------------------------------------------------------------------------------ NT, bf16, 8 waves, 8-phase K-loop (256 x 256 x 64 and relatives)
// The 128 x 128 kernel above asks the CU's vector-memory path for 32 KB per 64-deep k-step and workgroup -- 60 B per clock and CU at matrix-pipe
// speed against the 64 B per clock the texture / L1 path is specified at (round 3: TA busy 54-68 %, TCP_PENDING_STALL ~50 % of the launch) --
// and runs its whole workgroup in lockstep (DMA issue, barrier, fragment reads, MFMAs).  This kernel halves the operand bytes per FLOP (256 x 256
// tile: 64 KB per k-step for 4x the MFMAs) and replaces the lockstep by the phase schedule of cdna_hip_programming.md 5 ("256^2 8-phase template"):
//   * 8 waves as 2 (M) x 4 (N); a wave owns (2 HM) x (HN0 + HN1) accumulator tiles of 16 x 16 -- 8 x 4 for the 256 x 256 tile, 6 x 4 for
//     192 x 256, 6 x 5 for 192 x 320; one workgroup per CU, two k-tile buffers of {A0, A1, B0, B1} half-tiles in LDS (128 KB at most).  Half h
//     of A holds the rows {wr * 2 HM 16 + h * HM 16 + r} of both wave rows, half h of B the columns of all four wave columns: every wave reads
//     ITS part of a half-tile, and a half-tile is free for its refill as soon as the one phase that reads it is over.
//   * a k-tile is four phases, one accumulator quadrant (HM x HNh tiles x K 64: 16 MFMAs at 256 x 256) each: (A0, B0) -> (A0, B1) -> (A1, B1) ->
//     (A1, B0); a phase is {fragment reads of the half-tile(s) it needs, ONE half-tile refill (2-3 LDS-DMA instructions per thread), barrier,
//     its MFMAs at raised priority, barrier}.  The refills run two k-tiles ahead; the only vmcnt wait is in phase 4 and leaves the three
//     youngest half-tiles in flight -- never zero inside the loop.
//   * the two wave rows run half a phase apart (wr == 1 takes one extra barrier up front, wr == 0 one at the end): while one wave of a SIMD
//     issues its MFMAs the other reads fragments and issues DMA, so the matrix pipe sees a new MFMA group as soon as the last one drains.
// Hazards (who may touch which half-tile when): a refill targets a half-tile whose last reads were retired by an lgkmcnt wait at least one barrier
// earlier in EVERY wave (B0: the counted lgkmcnt of phase 1, refilled in phase 2; A0 / B1 / A1: read in phase 1 / 2 / 3, refilled in phase
// 3 / 4 / 1); a half-tile is read one phase or more after the barrier that follows the vmcnt wait that retired its DMA in every wave (the wait
// of phase 4 covers k-tile t + 1 whole: the three half-tiles issued after its last one, A1(t + 1) in phase 1, are B0 / A0 / B1 of k-tile t + 2).
// Tile shapes: the launches of this model are 1.5 .. 10 tiles per CU, so whole rounds matter as much as the loop: 49152 x 512 is 384 tiles of
// 256 x 256 (1.5 rounds of 256 CUs) but 512 tiles of 192 x 256 (2 rounds of 3/4 the work each); 98304 x 320 is 512 tiles of 192 x 320.
// Preconditions (host dispatch): bf16, identity a_map, M % BM == 0, N % BN == 0, K % 64 == 0, lean epilogue (EPI 1-5; the 80-column wave
// tile of BN 320 carries EPI 1 / 2 only).
template <int EPI, int HM, int HN0, int HN1, bool RAG = false>
__global__ __launch_bounds__(512, 2) void gemm_nt_p8_kernel(mvlt_gemm_nt_args p) {
  // RAG: M and / or N are not whole tiles (the MLM logits: ~1500 selected rows x 30522 words).  The loader then points the rows past the end at
  // the last valid row -- their products are never stored: the epilogue runs with its bound checks -- which costs nothing inside the K-loop.
  constexpr int WMT = 2 * HM, WNT = HN0 + HN1;                    // accumulator tiles per wave
  constexpr int BMT = 2 * WMT * 16, BNT = 4 * WNT * 16;           // workgroup tile
  constexpr int AH = 2 * HM * 16, BH0 = 4 * HN0 * 16, BH1 = 4 * HN1 * 16;      // rows of the A / B0 / B1 half-tiles
  constexpr int A_IT = (AH + 63) / 64, B_IT0 = BH0 / 64, B_IT1 = BH1 / 64;     // DMA instructions per thread (the last A one: waves 0-3 only when AH = 96)
  constexpr bool A_PART = AH % 64 != 0;
  static_assert(BH0 % 64 == 0 && BH1 % 64 == 0 && (!A_PART || AH % 64 == 32), "half-tile geometry");
  constexpr int OFF_A1 = AH * 128, OFF_B0 = 2 * AH * 128, OFF_B1 = OFF_B0 + BH0 * 128, BUF = OFF_B1 + BH1 * 128;
  extern __shared__ __attribute__((aligned(16))) char smem[];     // [2 buffers][A0 | A1 | B0 | B1]
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wr = wave >> 2, wc = wave & 3;
  const int tiles_m = RAG ? (p.M + BMT - 1) / BMT : p.M / BMT, tiles_n = RAG ? (p.N + BNT - 1) / BNT : p.N / BNT;
  const int bid = blockIdx.x;
  const int xcd = bid & 7, bslot = bid >> 3;
  const int tile_m = (bslot / tiles_n) * 8 + xcd, tile_n = bslot % tiles_n;      // the n-tiles of an m-tile are neighbours on one XCD
  if (tile_m >= tiles_m) return;
  const int m0 = tile_m * BMT, n0 = tile_n * BNT;
  const unsigned smem_lds = (unsigned)(uintptr_t)smem;
  const int nk = p.K >> 6;

  // ---- loader: DMA instruction i of a half-tile covers its rows 64 i .. 64 i + 63, thread -> (row (tid >> 3) + 64 i, slot tid & 7); the slot holds
  //      source chunk slot ^ ((row >> 1) & 7) (the read-side swizzle, an involution; rows 64 apart share the mask).  Source address = a scalar
  //      base per (operand, half, k-tile) + a per-thread 32-bit offset per instruction.
  const int lrow = tid >> 3;
  const int chunk = (tid & 7) ^ ((lrow >> 1) & 7);
  const unsigned a_rs = 2u * (unsigned)p.lda, b_rs = 2u * (unsigned)p.ldb;
  unsigned a_voff[A_IT], a_voff1[RAG ? A_IT : 1], b_voff0[B_IT0], b_voff1[B_IT1];
#pragma unroll
  for (int i = 0; i < A_IT; ++i) {
    const int lr = lrow + 64 * i, w_ = lr / (HM * 16), rem = lr - w_ * (HM * 16);
    const int trow = w_ * (WMT * 16) + rem;                     // row inside the tile, half 0; half 1 is HM * 16 rows further
    a_voff[i] = (unsigned)(RAG ? min(trow, p.M - 1 - m0) : trow) * a_rs + chunk * 16;
    if (RAG) a_voff1[i] = (unsigned)min(trow + HM * 16, p.M - 1 - m0) * a_rs + chunk * 16;
  }
#pragma unroll
  for (int i = 0; i < B_IT0; ++i) {
    const int lr = lrow + 64 * i, w_ = lr / (HN0 * 16), rem = lr - w_ * (HN0 * 16);
    const int trow = w_ * (WNT * 16) + rem;
    b_voff0[i] = (unsigned)(RAG ? min(trow, p.N - 1 - n0) : trow) * b_rs + chunk * 16;
  }
#pragma unroll
  for (int i = 0; i < B_IT1; ++i) {
    const int lr = lrow + 64 * i, w_ = lr / (HN1 * 16), rem = lr - w_ * (HN1 * 16);
    const int trow = w_ * (WNT * 16) + HN0 * 16 + rem;
    b_voff1[i] = (unsigned)(RAG ? min(trow, p.N - 1 - n0) : trow) * b_rs + chunk * 16;
  }
  const char* const a_base = (const char*)p.A + (size_t)m0 * a_rs;
  const char* const b_base = (const char*)p.B + (size_t)n0 * b_rs;
  const unsigned dst_wave = smem_lds + wave * 1024;
  // which: 0 = A0, 1 = A1, 2 = B0, 3 = B1 (compile-time at every call site)
  auto stage = [&](int which, int t, int buf) {
    if (which < 2) {
      const char* sb = a_base + (RAG ? (size_t)0 : (size_t)(which * HM * 16) * a_rs) + t * 128;
      const unsigned dst = dst_wave + buf * BUF + which * OFF_A1;
#pragma unroll
      for (int i = 0; i < A_IT; ++i)
        if (!A_PART || i + 1 < A_IT || wave < 4) glds16_s(sb, (RAG && which == 1) ? a_voff1[i] : a_voff[i], dst + i * 8192);
    } else if (which == 2) {
      const char* sb = b_base + t * 128;
      const unsigned dst = dst_wave + buf * BUF + OFF_B0;
#pragma unroll
      for (int i = 0; i < B_IT0; ++i) glds16_s(sb, b_voff0[i], dst + i * 8192);
    } else {
      const char* sb = b_base + t * 128;
      const unsigned dst = dst_wave + buf * BUF + OFF_B1;
#pragma unroll
      for (int i = 0; i < B_IT1; ++i) glds16_s(sb, b_voff1[i], dst + i * 8192);
    }
  };
  // DMA instructions of THIS wave in the three youngest half-tiles (B0, A0, B1) = what the wait of phase 4 leaves in flight
  constexpr int INFL0 = B_IT0 + A_IT + B_IT1, INFL1 = B_IT0 + (A_PART ? A_IT - 1 : A_IT) + B_IT1;
  auto wait_tile = [&](bool more) {
    if (!more) wait_vm<0>();
    else if (wr == 0) wait_vm<INFL0>();
    else wait_vm<INFL1>();
  };

  // ---- fragment geometry: lane (fr, fg) reads row fr of a 16-row tile, chunk (ks * 4 + fg) ^ ((fr >> 1) & 7)
  const int fr = lane & 15, fg = lane >> 4;
  const int sw = (fr >> 1) & 7;
  const char* const fa_base = smem + (wr * HM * 16 + fr) * 128;
  const char* const fb0_base = smem + OFF_B0 + (wc * HN0 * 16 + fr) * 128;
  const char* const fb1_base = smem + OFF_B1 + (wc * HN1 * 16 + fr) * 128;
  const int koff0 = ((fg ^ sw) & 7) << 4, koff1 = (((4 + fg) ^ sw) & 7) << 4;

  f32x4 acc[WMT][WNT];
#pragma unroll
  for (int i = 0; i < WMT; ++i)
#pragma unroll
    for (int j = 0; j < WNT; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
  u32x4 fa[2][HM], fb0[2][HN0], fb1[2][HN1];

#define MVLT_LDA(BUFI, MH)                                                                                         \
  _Pragma("unroll") for (int i = 0; i < HM; ++i) {                                                                 \
    fa[0][i] = *(const u32x4*)(fa_base + (BUFI) * BUF + (MH) * OFF_A1 + i * 2048 + koff0);                         \
    fa[1][i] = *(const u32x4*)(fa_base + (BUFI) * BUF + (MH) * OFF_A1 + i * 2048 + koff1);                         \
  }
#define MVLT_LDB0(BUFI)                                                                                            \
  _Pragma("unroll") for (int j = 0; j < HN0; ++j) {                                                                \
    fb0[0][j] = *(const u32x4*)(fb0_base + (BUFI) * BUF + j * 2048 + koff0);                                       \
    fb0[1][j] = *(const u32x4*)(fb0_base + (BUFI) * BUF + j * 2048 + koff1);                                       \
  }
#define MVLT_LDB1(BUFI)                                                                                            \
  _Pragma("unroll") for (int j = 0; j < HN1; ++j) {                                                                \
    fb1[0][j] = *(const u32x4*)(fb1_base + (BUFI) * BUF + j * 2048 + koff0);                                       \
    fb1[1][j] = *(const u32x4*)(fb1_base + (BUFI) * BUF + j * 2048 + koff1);                                       \
  }
#define MVLT_MMA(MH, JBASE, HN, FB)                                                                                \
  do {                                                                                                             \
    __builtin_amdgcn_s_setprio(1);                                                                                 \
    _Pragma("unroll") for (int ks = 0; ks < 2; ++ks)                                                               \
      _Pragma("unroll") for (int i = 0; i < HM; ++i)                                                               \
        _Pragma("unroll") for (int j = 0; j < (HN); ++j)                                                           \
          acc[(MH) * HM + i][(JBASE) + j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(                               \
              __builtin_bit_cast(bf16x8, fa[ks][i]), __builtin_bit_cast(bf16x8, FB[ks][j]), acc[(MH) * HM + i][(JBASE) + j], 0, 0, 0); \
    __builtin_amdgcn_s_setprio(0);                                                                                 \
  } while (0)

  // ---- prologue: k-tile 0 whole, and the first three half-tiles of k-tile 1, in the loop's own issue order (B0, A0, B1, A1)
  stage(2, 0, 0); stage(0, 0, 0); stage(3, 0, 0); stage(1, 0, 0);
  if (nk > 1) { stage(2, 1, 1); stage(0, 1, 1); stage(3, 1, 1); }
  wait_tile(nk > 1);
  MVLT_BAR();
  if (wr == 1) MVLT_BAR();                        // the second wave row runs half a phase behind the first

  auto ktile = [&](auto bufc, int t) {
    constexpr int B = decltype(bufc)::value;
    // phase 1: quadrant (0, 0); refill A1 of k-tile t + 1 (other buffer: last read in phase 3 of k-tile t - 1)
    MVLT_LDB0(B)
    __builtin_amdgcn_sched_barrier(0);
    MVLT_LDA(B, 0)
    __builtin_amdgcn_sched_barrier(0);
    if (t + 1 < nk) stage(1, t + 1, B ^ 1);
    wait_lgkm<2 * HM>();                          // the B0 reads (issued first) are back: B0 may be refilled in phase 2
    MVLT_BAR();
    MVLT_MMA(0, 0, HN0, fb0);
    MVLT_BAR();
    // phase 2: quadrant (0, 1); refill B0 of k-tile t + 2
    MVLT_LDB1(B)
    __builtin_amdgcn_sched_barrier(0);
    if (t + 2 < nk) stage(2, t + 2, B);
    MVLT_BAR();
    MVLT_MMA(0, HN0, HN1, fb1);
    MVLT_BAR();
    // phase 3: quadrant (1, 1); refill A0 of k-tile t + 2
    MVLT_LDA(B, 1)
    __builtin_amdgcn_sched_barrier(0);
    if (t + 2 < nk) stage(0, t + 2, B);
    MVLT_BAR();
    MVLT_MMA(1, HN0, HN1, fb1);
    MVLT_BAR();
    // phase 4: quadrant (1, 0) from registers; refill B1 of k-tile t + 2; k-tile t + 1 must have landed when this phase ends
    if (t + 2 < nk) stage(3, t + 2, B);
    wait_tile(t + 2 < nk);
    MVLT_BAR();
    MVLT_MMA(1, 0, HN0, fb0);
    MVLT_BAR();
  };
  for (int t = 0; t < nk; t += 2) {
    ktile(std::integral_constant<int, 0>{}, t);
    if (t + 1 < nk) ktile(std::integral_constant<int, 1>{}, t + 1);
  }
  if (wr == 0) MVLT_BAR();
  MVLT_BAR();                                      // every wave is out of the loop: the epilogue may reuse the LDS
  // (whole tiles only: the bound checks go, -20 us on the GELU' launches; not for the residual epilogue, which measured 9 us SLOWER without them --
  //  49152 x 512 x 2048 + R 120 -> 129 us, same box, two passes: its prefetched rows are then requested in a different order)
  if constexpr (WNT == 4) nt_epilogue_lean<128, EPI, WMT, 4, EPI != 2 && !RAG>(p, acc, smem, m0, n0, wave, lane);
  else nt_epilogue_w80<EPI, WMT, RAG>(p, acc, smem, m0, n0, wave, lane);
}

}  // namespace

// ------------------------------------------------------------------------------------------------ plan -> launch
int mvlt_launch_nt_p8(const mvlt_gemm_plan& p, const mvlt_gemm_nt_args& a, hipStream_t s) {
  const char* const who = "mvlt_gemm_nt";
  MVLT_PLAN_LAUNCH_HEAD;
#define NT_P8(EPI_, HM_, HN0_, HN1_, RAG_) MVLT_CASE(true, (gemm_nt_p8_kernel<EPI_, HM_, HN0_, HN1_, RAG_>), (MVLT_GEMM_NT_P8, EPI_, HM_, HN0_, HN1_, RAG_), a)
  switch (key) {
    NT_P8(1, 4, 2, 2, true) NT_P8(1, 3, 3, 2, true) NT_P8(2, 3, 3, 2, true) NT_P8(1, 3, 3, 2, false) NT_P8(2, 3, 3, 2, false)
    NT_P8(1, 4, 2, 2, false) NT_P8(2, 4, 2, 2, false) NT_P8(3, 4, 2, 2, false) NT_P8(4, 4, 2, 2, false) NT_P8(5, 4, 2, 2, false)
    NT_P8(1, 3, 2, 2, false) NT_P8(2, 3, 2, 2, false) NT_P8(3, 3, 2, 2, false) NT_P8(4, 3, 2, 2, false) NT_P8(5, 3, 2, 2, false)
  }
  return no_instantiation(who, p);
}

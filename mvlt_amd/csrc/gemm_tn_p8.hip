// TN GEMM (weight gradients), bf16, 8 waves, 8-phase loop.  Overview: gemm.hip.
#include "gemm_common.h"

namespace {

// ------------------------------------------------------------------------------------------------ TN (weight gradients), bf16, 8 waves, 8-phase loop
// C[N1, N2] += A[M, N1]^T B[M, N2] on the schedule of gemm_nt_p8_kernel: the reduction runs over the ROWS of both operands (k-tile = 64 rows), the
// operand tiles keep their natural [m][n] layout in LDS (LDS-DMA cannot transpose) and the MFMA fragments -- 8 consecutive m of one n per lane --
// come from two ds_read_b64_tr_b16 each, as in gemm_tn_dma_kernel.  Half h of A holds the columns {wr * 2 HM 16 + h * HM 16 + c} of both wave rows
// as a [64 m][2 HM 16] image, half h of B the columns of all four wave columns as [64 m][4 HNh 16]; row pitches 128 / 256 / 384 B, the 16-byte
// chunks of a row XOR-ed (on the source side) with a hash of the row so that the eight rows a 32-lane transposed read touches (m .. m+3, m+8 ..
// m+11) fall into eight different 32-byte bank windows: pitch 256 -> (row & 3) | bit 3 of the row; pitch 128 and 384 (both 4 windows mod 8 per
// row) -> bit 1 | bit 3.  Tiles: 256 x 256 (2048 x 512 at stage 4) and 128 x 320 (1280 x 320 at stage 3); an output whose 320-multiple side is N1 is
// computed as its transpose (operands swapped by the host, the MFMA operand order flipped so that a lane's 16 consecutive outputs stay contiguous
// in memory).  The m range is split over workgroups (one per CU), partial tiles meet by fp32 atomics; bias gradients = ones-fragment MFMAs,
// taken in turns by the workgroups that share an operand column range.
template <int PITCH> __device__ __forceinline__ int tn_hash(int row) {
  // pitch 192 (round 6, the 96-column A half-tile of the 192 x 320 tile): a row advances 6 windows mod 8, so rows m .. m+3 sit in windows {0, 6, 4, 2} + w and rows
  // m+8 .. m+11 in the same ones: bit 3 of the row flips the window's low bit ({1, 7, 5, 3} + w) -- eight distinct windows for either read of a fragment
  if (PITCH == 192) return (row >> 3) & 1;
  return PITCH == 256 ? ((row & 3) | (((row >> 3) & 1) << 2)) : (((row >> 1) & 1) | (((row >> 3) & 1) << 1));
}
// Round 6: the 192 x 320 tile (<3, 3, 2>: 30 accumulator tiles per wave, as in gemm_nt_p8_kernel) for the fc weight gradients of stage 3 -- 1280 x 320 and 320 x 1280 over
// 98304 (pvlt_medium at 384 px: 45056) rows.  The 320 side is one column tile; the 1280 side is 6.67 row tiles: RAG1 = the last row tile is ragged (its loader columns are
// clamped to the last 8 valid ones, its rows / column sums past N1 are not stored: 7 tiles for 6.67 of work).  SWAP = the caller's N1 is the 320 side: the host swaps the
// operands (A' = B, B' = A) and this instantiation stores its partial tiles TRANSPOSED, i.e. in the caller's [N1][N2] layout (needs the un-flipped MFMA operand order: a
// lane then owns four consecutive kernel-n1 = caller-n2 of one caller-n1).
template <int HM, int HN0, int HN1, bool TRANS, bool RAG1 = false, bool SWAP = false>
__global__ __launch_bounds__(512, 2) void gemm_tn_p8_kernel(mvlt_gemm_tn_args p, int kt_per, int t1, int t2, int splits, bf16* part) {
  constexpr int WMT = 2 * HM, WNT = HN0 + HN1;
  constexpr int AC = 2 * HM * 16, BC0 = 4 * HN0 * 16, BC1 = 4 * HN1 * 16;          // columns of the A / B0 / B1 half-tiles
  constexpr int PA = AC * 2, PB0 = BC0 * 2, PB1 = BC1 * 2;                         // row pitches in bytes
  constexpr int A_IT = (64 * PA + 8191) / 8192, B_IT0 = 64 * PB0 / 8192, B_IT1 = 64 * PB1 / 8192;
  constexpr bool A_PART = (64 * PA) % 8192 != 0;                                   // 12 KB half-tile: the second DMA instruction belongs to waves 0-3 only
  static_assert((PA == 128 || PA == 192 || PA == 256) && (PB0 == 256 || PB0 == 384) && PB1 == 256, "half-tile pitches with a bank hash");
  static_assert(!SWAP || !TRANS, "the transposed partial store needs the un-flipped accumulator layout");
  constexpr int OFF_A1 = 64 * PA, OFF_B0 = 2 * 64 * PA, OFF_B1 = OFF_B0 + 64 * PB0, BUF = OFF_B1 + 64 * PB1;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wr = wave >> 2, wc = wave & 3;
  // all output tiles of one m-split on ONE XCD (workgroup b runs on XCD b % 8): the operand rows pass that L2 once
  const int txy = t1 * t2;
  int bz, xy;
  if (splits >= 8) {
    const int xcd = blockIdx.x & 7, kq = blockIdx.x >> 3;
    const int zq = kq / txy;
    xy = kq - zq * txy;
    bz = zq * 8 + xcd;
    if (bz >= splits) return;
  } else {
    bz = blockIdx.x / txy;
    xy = blockIdx.x - bz * txy;
  }
  const int bx = xy % t1, by = xy / t1;
  const int n1_0 = bx * (2 * WMT * 16), n2_0 = by * (4 * WNT * 16);
  const int nkt = p.M >> 6;
  const int kt0 = bz * kt_per;
  const int nk = min(kt_per, nkt - kt0);
  if (nk <= 0) return;
  const unsigned smem_lds = (unsigned)(uintptr_t)smem;
  const unsigned a_rs = 2u * (unsigned)p.lda, b_rs = 2u * (unsigned)p.ldb;

  // ---- loader: chunk q = tid + 512 i of a half-tile = (row q / CPR, slot q % CPR); the slot holds source chunk slot ^ (hash(row) << 1)
  unsigned a_voff[A_IT], a_voff1[RAG1 ? A_IT : 1], b_voff0[B_IT0], b_voff1[B_IT1];
#pragma unroll
  for (int i = 0; i < A_IT; ++i) {
    constexpr int CPR = PA / 16;
    const int q = tid + 512 * i, row = (q / CPR) & 63, lc = ((q - (q / CPR) * CPR) ^ (tn_hash<PA>(row) << 1)) * 8;      // (& 63: the idle half of a partial instruction)
    const int w_ = lc / (HM * 16);
    const int col = w_ * (WMT * 16) + (lc - w_ * (HM * 16));                      // column inside the tile, half 0; half 1 is HM * 16 further
    a_voff[i] = (unsigned)row * a_rs + 2u * (unsigned)(RAG1 ? min(col, p.N1 - 8 - n1_0) : col);
    if (RAG1) a_voff1[i] = (unsigned)row * a_rs + 2u * (unsigned)min(col + HM * 16, p.N1 - 8 - n1_0);
  }
#pragma unroll
  for (int i = 0; i < B_IT0; ++i) {
    constexpr int CPR = PB0 / 16;
    const int q = tid + 512 * i, row = q / CPR, lc = ((q - row * CPR) ^ (tn_hash<PB0>(row) << 1)) * 8;
    const int w_ = lc / (HN0 * 16);
    b_voff0[i] = (unsigned)row * b_rs + 2u * (unsigned)(w_ * (WNT * 16) + (lc - w_ * (HN0 * 16)));
  }
#pragma unroll
  for (int i = 0; i < B_IT1; ++i) {
    constexpr int CPR = PB1 / 16;
    const int q = tid + 512 * i, row = q / CPR, lc = ((q - row * CPR) ^ (tn_hash<PB1>(row) << 1)) * 8;
    const int w_ = lc / (HN1 * 16);
    b_voff1[i] = (unsigned)row * b_rs + 2u * (unsigned)(w_ * (WNT * 16) + HN0 * 16 + (lc - w_ * (HN1 * 16)));
  }
  const char* const a_base = (const char*)p.A + (size_t)(kt0 * 64) * a_rs + (size_t)n1_0 * 2;
  const char* const b_base = (const char*)p.B + (size_t)(kt0 * 64) * b_rs + (size_t)n2_0 * 2;
  const unsigned dst_wave = smem_lds + wave * 1024;
  auto stage = [&](int which, int t, int buf) {
    if (which < 2) {
      const char* sb = a_base + (size_t)(t * 64) * a_rs + (RAG1 ? 0 : which * (HM * 16 * 2));
      const unsigned dst = dst_wave + buf * BUF + which * OFF_A1;
#pragma unroll
      for (int i = 0; i < A_IT; ++i)
        if (!A_PART || i + 1 < A_IT || wave < 4) glds16_s(sb, (RAG1 && which == 1) ? a_voff1[i] : a_voff[i], dst + i * 8192);
    } else if (which == 2) {
      const char* sb = b_base + (size_t)(t * 64) * b_rs;
      const unsigned dst = dst_wave + buf * BUF + OFF_B0;
#pragma unroll
      for (int i = 0; i < B_IT0; ++i) glds16_s(sb, b_voff0[i], dst + i * 8192);
    } else {
      const char* sb = b_base + (size_t)(t * 64) * b_rs;
      const unsigned dst = dst_wave + buf * BUF + OFF_B1;
#pragma unroll
      for (int i = 0; i < B_IT1; ++i) glds16_s(sb, b_voff1[i], dst + i * 8192);
    }
  };
  // DMA instructions of THIS wave in the three youngest half-tiles (B0, A0, B1): what the wait of phase 4 leaves in flight
  constexpr int INFL0 = B_IT0 + A_IT + B_IT1, INFL1 = B_IT0 + (A_PART ? A_IT - 1 : A_IT) + B_IT1;
  auto wait_infl = [&]() { if (wr == 0) wait_vm<INFL0>(); else wait_vm<INFL1>(); };

  // ---- fragment geometry (transposed reads): lane (g, L) supplies k-row 8 g + (L >> 2) and the row 4 below, 8-byte piece L & 3 of a 16-column
  //      window; the k32 step ks adds 32 rows
  const int g = lane >> 4, L = lane & 15;
  const int frow = 8 * g + (L >> 2);
  int aoff[HM], boff0[HN0], boff1[HN1];
#pragma unroll
  for (int i = 0; i < HM; ++i) aoff[i] = frow * PA + (((wr * HM + i) ^ tn_hash<PA>(frow)) << 5) + ((L & 3) << 3);
#pragma unroll
  for (int j = 0; j < HN0; ++j) boff0[j] = OFF_B0 + frow * PB0 + (((wc * HN0 + j) ^ tn_hash<PB0>(frow)) << 5) + ((L & 3) << 3);
#pragma unroll
  for (int j = 0; j < HN1; ++j) boff1[j] = OFF_B1 + frow * PB1 + (((wc * HN1 + j) ^ tn_hash<PB1>(frow)) << 5) + ((L & 3) << 3);

  f32x4 acc[WMT][WNT];
#pragma unroll
  for (int i = 0; i < WMT; ++i)
#pragma unroll
    for (int j = 0; j < WNT; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
  // bias gradients: column sums of A (colsum_a) or of B (colsum_b) by one MFMA against an all-ones fragment.  The A fragments of accumulator row tile
  // i are read by the four waves of a wave row: wave wc takes i == wc; the B fragments of column tile j by the two wave rows: j & 1 == wr.
  f32x4 csa[2] = {f32x4{0.f, 0.f, 0.f, 0.f}, f32x4{0.f, 0.f, 0.f, 0.f}};
  f32x4 csb[(WNT + 1) / 2];
#pragma unroll
  for (int j = 0; j < (WNT + 1) / 2; ++j) csb[j] = f32x4{0.f, 0.f, 0.f, 0.f};
  const bf16x8 ones = __builtin_bit_cast(bf16x8, u32x4{0x3F803F80u, 0x3F803F80u, 0x3F803F80u, 0x3F803F80u});
  const bool do_csa = p.colsum_a != nullptr, do_csb = p.colsum_b != nullptr;
  u32x4 fa[2][HM], fb0[2][HN0], fb1[2][HN1];

#define MVLT_TLDA(BUFI, MH)                                                                                        \
  _Pragma("unroll") for (int i = 0; i < HM; ++i) {                                                                 \
    fa[0][i] = tr_frag(smem + (BUFI) * BUF + (MH) * OFF_A1 + aoff[i], PA);                                         \
    fa[1][i] = tr_frag(smem + (BUFI) * BUF + (MH) * OFF_A1 + aoff[i] + 32 * PA, PA);                               \
  }
#define MVLT_TLDB0(BUFI)                                                                                           \
  _Pragma("unroll") for (int j = 0; j < HN0; ++j) {                                                                \
    fb0[0][j] = tr_frag(smem + (BUFI) * BUF + boff0[j], PB0);                                                      \
    fb0[1][j] = tr_frag(smem + (BUFI) * BUF + boff0[j] + 32 * PB0, PB0);                                           \
  }
#define MVLT_TLDB1(BUFI)                                                                                           \
  _Pragma("unroll") for (int j = 0; j < HN1; ++j) {                                                                \
    fb1[0][j] = tr_frag(smem + (BUFI) * BUF + boff1[j], PB1);                                                      \
    fb1[1][j] = tr_frag(smem + (BUFI) * BUF + boff1[j] + 32 * PB1, PB1);                                           \
  }
#define MVLT_TMMA(MH, JBASE, HN, FB)                                                                               \
  _Pragma("unroll") for (int ks = 0; ks < 2; ++ks)                                                                 \
    _Pragma("unroll") for (int i = 0; i < HM; ++i)                                                                 \
      _Pragma("unroll") for (int j = 0; j < (HN); ++j) {                                                           \
        f32x4& c_ = acc[(MH) * HM + i][(JBASE) + j];                                                               \
        if (TRANS) c_ = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, FB[ks][j]), __builtin_bit_cast(bf16x8, fa[ks][i]), c_, 0, 0, 0); \
        else c_ = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, fa[ks][i]), __builtin_bit_cast(bf16x8, FB[ks][j]), c_, 0, 0, 0);       \
      }
#define MVLT_TCSA(MH)                                                                                              \
  if (csa_now) {                                                                                                   \
    _Pragma("unroll") for (int ks = 0; ks < 2; ++ks)                                                               \
      _Pragma("unroll") for (int i = 0; i < HM; ++i)                                                               \
        if (i == wc) csa[MH] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, fa[ks][i]), ones, csa[MH], 0, 0, 0); \
  }
#define MVLT_TCSB(JBASE, HN, FB)                                                                                   \
  if (csb_now) {                                                                                                   \
    _Pragma("unroll") for (int ks = 0; ks < 2; ++ks)                                                               \
      _Pragma("unroll") for (int j = 0; j < (HN); ++j)                                                             \
        if ((((JBASE) + j) & 1) == wr) csb[((JBASE) + j) >> 1] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ones, __builtin_bit_cast(bf16x8, FB[ks][j]), csb[((JBASE) + j) >> 1], 0, 0, 0); \
  }

  stage(2, 0, 0); stage(0, 0, 0); stage(3, 0, 0); stage(1, 0, 0);
  if (nk > 1) { stage(2, 1, 1); stage(0, 1, 1); stage(3, 1, 1); wait_infl(); }
  else wait_vm<0>();
  MVLT_BAR();
  if (wr == 1) MVLT_BAR();

  auto ktile = [&](auto bufc, int t) {
    constexpr int B = decltype(bufc)::value;
    const bool csa_now = do_csa && (t % t2) == by, csb_now = do_csb && (t % t1) == bx;       // the workgroups sharing A (B) columns take turns
    MVLT_TLDB0(B)
    __builtin_amdgcn_sched_barrier(0);
    MVLT_TLDA(B, 0)
    __builtin_amdgcn_sched_barrier(0);
    if (t + 1 < nk) stage(1, t + 1, B ^ 1);
    wait_lgkm<(4 * HM < 15 ? 4 * HM : 15)>();     // the B0 reads (two 8-byte reads per fragment, issued first) are back (the counter has 4 bits)
    MVLT_BAR();
    __builtin_amdgcn_s_setprio(1);
    MVLT_TMMA(0, 0, HN0, fb0)
    MVLT_TCSA(0)
    MVLT_TCSB(0, HN0, fb0)
    __builtin_amdgcn_s_setprio(0);
    MVLT_BAR();
    MVLT_TLDB1(B)
    __builtin_amdgcn_sched_barrier(0);
    if (t + 2 < nk) stage(2, t + 2, B);
    MVLT_BAR();
    __builtin_amdgcn_s_setprio(1);
    MVLT_TMMA(0, HN0, HN1, fb1)
    MVLT_TCSB(HN0, HN1, fb1)
    __builtin_amdgcn_s_setprio(0);
    MVLT_BAR();
    MVLT_TLDA(B, 1)
    __builtin_amdgcn_sched_barrier(0);
    if (t + 2 < nk) stage(0, t + 2, B);
    MVLT_BAR();
    __builtin_amdgcn_s_setprio(1);
    MVLT_TMMA(1, HN0, HN1, fb1)
    MVLT_TCSA(1)
    __builtin_amdgcn_s_setprio(0);
    MVLT_BAR();
    if (t + 2 < nk) { stage(3, t + 2, B); wait_infl(); }
    else wait_vm<0>();
    MVLT_BAR();
    __builtin_amdgcn_s_setprio(1);
    MVLT_TMMA(1, 0, HN0, fb0)
    __builtin_amdgcn_s_setprio(0);
    MVLT_BAR();
  };
  for (int t = 0; t < nk; t += 2) {
    ktile(std::integral_constant<int, 0>{}, t);
    if (t + 1 < nk) ktile(std::integral_constant<int, 1>{}, t + 1);
  }
  if (wr == 0) MVLT_BAR();
  const int fr = lane & 15, fg = lane >> 4;
  if (do_csa && fr == 0 && wc < HM) {            // csa[mh][r]: column n1 = tile (mh * HM + wc), row 4 fg + r of it (identical in every lane column)
#pragma unroll
    for (int mh = 0; mh < 2; ++mh)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int n1 = n1_0 + wr * (WMT * 16) + (mh * HM + wc) * 16 + 4 * fg + r;
        if (!RAG1 || n1 < p.N1) atomicAdd(&p.colsum_a[n1], csa[mh][r]);
      }
  }
  if (do_csb && fg == 0) {                        // csb[j >> 1][0]: column n2 = tile j, lane column fr
#pragma unroll
    for (int j = 0; j < WNT; ++j)
      if ((j & 1) == wr) atomicAdd(&p.colsum_b[n2_0 + wc * (WNT * 16) + j * 16 + fr], csb[j >> 1][0]);
  }
  if constexpr (SWAP) {
    // PARTIAL-TILE mode, operands swapped by the host (kernel n1 = the caller's n2 and vice versa): the split's tile goes to part[split][caller N1 = p.N2][caller N2 = p.N1],
    // the caller's layout, so that the same fold serves it.  Un-flipped accumulators: acc[i][j][r] = C'[n1 = tile i row 4 fg + r][n2 = tile j column fr]: a lane owns four
    // consecutive kernel-n1 of one kernel-n2 = four consecutive columns of one row of the caller's matrix.  Per wave and kernel-n2 tile j: a [16 n2][WMT * 16 n1] LDS tile,
    // out as whole 16-byte pieces of contiguous rows.
    bf16* const P = part + (size_t)bz * p.N1 * p.N2;
    constexpr int LDP = WMT * 16 + 8;
    constexpr int CPR = WMT * 2;
    MVLT_BAR();
    bf16* const st = (bf16*)smem + wave * 16 * LDP;
#pragma unroll
    for (int j = 0; j < WNT; ++j) {
      __builtin_amdgcn_wave_barrier();
#pragma unroll
      for (int i = 0; i < WMT; ++i) {
        const bf16x2 lo = __builtin_convertvector(f32x2{acc[i][j][0], acc[i][j][1]}, bf16x2), hi = __builtin_convertvector(f32x2{acc[i][j][2], acc[i][j][3]}, bf16x2);
        *(u32x2*)(st + fr * LDP + i * 16 + 4 * fg) = u32x2{__builtin_bit_cast(unsigned, lo), __builtin_bit_cast(unsigned, hi)};
      }
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
      __builtin_amdgcn_wave_barrier();
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
#pragma unroll
      for (int q = lane; q < 16 * CPR; q += 64) {
        const int row = q / CPR, ch = q - row * CPR;
        const int n2 = n2_0 + wc * (WNT * 16) + j * 16 + row, n1 = n1_0 + wr * (WMT * 16) + ch * 8;
        if (!RAG1 || n1 < p.N1) st_g<MVLT_NT_GEMM>((u32x4*)(P + (size_t)n2 * p.N1 + n1), *(const u32x4*)(st + row * LDP + ch * 8));
      }
    }
    return;
  } else if (part) {
    // PARTIAL-TILE mode (round 5): no atomics.  The split's tile goes to part[split][N1][N2] in bf16 -- the MFMA operands are flipped (TRANS instantiation), so a lane owns
    // four consecutive n2 of one n1: one 8-byte store per accumulator tile -- and tn_fold_kernel adds the splits' tiles into C in a fixed order (deterministic).
    static_assert(TRANS, "partial tiles are stored from the flipped accumulator layout");
    bf16* const P = part + (size_t)bz * p.N1 * p.N2;
    // through a per-wave LDS tile [16 n1][WNT * 16 n2] so that the partial tile leaves as whole 16-byte pieces of contiguous rows (8-byte pieces 32 B apart cost 22 us per launch)
    constexpr int LDP = WNT * 16 + 8;              // bf16 elements per staged row (16 B of padding)
    constexpr int CPR = WNT * 2;                   // 16-byte chunks per row
    MVLT_BAR();                                    // every wave is out of the loop: the k-tile buffers are free
    bf16* const st = (bf16*)smem + wave * 16 * LDP;
#pragma unroll
    for (int i = 0; i < WMT; ++i) {
      __builtin_amdgcn_wave_barrier();
#pragma unroll
      for (int j = 0; j < WNT; ++j) {
        const bf16x2 lo = __builtin_convertvector(f32x2{acc[i][j][0], acc[i][j][1]}, bf16x2), hi = __builtin_convertvector(f32x2{acc[i][j][2], acc[i][j][3]}, bf16x2);
        *(u32x2*)(st + fr * LDP + j * 16 + 4 * fg) = u32x2{__builtin_bit_cast(unsigned, lo), __builtin_bit_cast(unsigned, hi)};
      }
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
      __builtin_amdgcn_wave_barrier();
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
#pragma unroll
      for (int q = lane; q < 16 * CPR; q += 64) {
        const int row = q / CPR, ch = q - row * CPR;
        const int n1 = n1_0 + wr * (WMT * 16) + i * 16 + row, n2 = n2_0 + wc * (WNT * 16) + ch * 8;
        if (!RAG1 || n1 < p.N1) st_g<MVLT_NT_GEMM>((u32x4*)(P + (size_t)n1 * p.N2 + n2), *(const u32x4*)(st + row * LDP + ch * 8));
      }
    }
    return;
  }
#pragma unroll
  for (int i = 0; i < WMT; ++i)
#pragma unroll
    for (int j = 0; j < WNT; ++j)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        if (TRANS) {                              // acc[r] = C[n2 tile j row 4 fg + r][n1 tile i column fr], stored transposed: consecutive lanes = consecutive n1
          const int n2 = n2_0 + wc * (WNT * 16) + j * 16 + 4 * fg + r, n1 = n1_0 + wr * (WMT * 16) + i * 16 + fr;
          atomicAdd(&p.C[(long)n2 * p.ldc + n1], acc[i][j][r]);
        } else {
          const int n1 = n1_0 + wr * (WMT * 16) + i * 16 + 4 * fg + r, n2 = n2_0 + wc * (WNT * 16) + j * 16 + fr;
          atomicAdd(&p.C[(long)n1 * p.ldc + n2], acc[i][j][r]);
        }
      }
}

}  // namespace

// ------------------------------------------------------------------------------------------------ plan -> launch
int mvlt_launch_tn_p8(const mvlt_gemm_plan& p, const mvlt_gemm_tn_args& k, bf16* part, hipStream_t s) {
  const char* const who = "mvlt_gemm_tn";
  MVLT_PLAN_LAUNCH_HEAD;
#define TN_P8(HM_, HN0_, HN1_, TRANS_, RAG1_, SWAP_) \
  MVLT_CASE(true, (gemm_tn_p8_kernel<HM_, HN0_, HN1_, TRANS_, RAG1_, SWAP_>), (MVLT_GEMM_TN_P8, HM_, HN0_, HN1_, TRANS_, RAG1_, SWAP_), k, p.per_split, p.t1, p.t2, p.splits, part)
  switch (key) {
    TN_P8(4, 2, 2, true, false, false)
    TN_P8(3, 3, 2, false, true, true) TN_P8(3, 3, 2, false, false, true) TN_P8(3, 3, 2, true, true, false) TN_P8(3, 3, 2, true, false, false)
  }
  return no_instantiation(who, p);
}

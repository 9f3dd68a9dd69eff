// TN GEMM (weight gradients), 4 waves: the register-staged kernel and the bf16 LDS-DMA kernel with its dgrad variant.  Overview: gemm.hip.
#include "gemm_common.h"

namespace {

// ------------------------------------------------------------------------------------------------ TN (wgrad)
// C[n1, n2] += sum_m A[m, n1] * B[m, n2].  The reduction index m is the slow (row) index of both operands, so
// tiles are transposed on their way into LDS (At[n1][m], Bt[n2][m], 64 m per tile) and the MFMA fragments again
// read 8 consecutive m.  The m range is split across gridDim.z; partial tiles are combined with fp32 atomics.

// bf16 transposed tiles hold (m, m+1) pairs as 32-bit words: row n = output index, 32 pair-columns.  Every 8 rows share
// the 4 low bank bits (row stride 144 B = 36 dwords), so the 16 lanes that write the same pair-column of 16 different
// row-groups would hit ONE bank; XOR-ing the pair-column with the row-group index (in units of 4 pairs = one 16-B
// fragment read, which therefore stays contiguous) spreads them over 8 banks (2-way on ds_write_b32 is free).
__device__ __forceinline__ int tsw(int n, int pair) { return pair ^ (((n >> 3) & 7) << 2); }

// destination column of logical output column n2 (mvlt_gemm_tn_args.c_taps / c_seg: [tap][cin] -> [cin][tap])
__device__ __forceinline__ int tn_dst_col(const mvlt_gemm_tn_args& p, int n2) {
  if (p.c_taps <= 1) return n2;
  const int tap = n2 / p.c_seg;
  return (n2 - tap * p.c_seg) * p.c_taps + tap;
}

template <typename T, int BN>
__global__ __launch_bounds__(NTHREADS) void gemm_tn_kernel(mvlt_gemm_tn_args p, int m_per_split) {
  constexpr int PC = Elem<T>::PER_CHUNK;             // elements per 16-B global chunk
  constexpr int ROWB = TElem<T>::ROWB;
  constexpr int WN = BN / 2;
  constexpr int TN_ = WN / 16;
  constexpr int A_CH = BM / PC;                      // chunks per tile row (A): 16 (bf16) / 32 (fp32)
  constexpr int B_CH = BN / PC;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  char* sA = smem;                                   // BM rows (n1) x ROWB
  char* sB = smem + BM * ROWB;                       // BN rows (n2) x ROWB
  float* s_colsum = (float*)(smem + (BM + BN) * ROWB);   // [BM]

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave >> 1, wn = wave & 1;
  const int n1_0 = blockIdx.x * BM, n2_0 = blockIdx.y * BN;
  const int m_begin = blockIdx.z * m_per_split;
  const int m_end = min(p.M, m_begin + m_per_split);
  const RowMap amap = to_rowmap(p.a_map), bmap = to_rowmap(p.b_map);
  const T* Ag = (const T*)p.A;
  const T* Bg = (const T*)p.B;
  const bool do_colsum = p.colsum_a != nullptr && blockIdx.y == 0;
  const bool do_colsum_b = p.colsum_b != nullptr && blockIdx.x == 0;
  if ((do_colsum || do_colsum_b) && tid < BM) s_colsum[tid] = 0.f;

  f32x4 acc[4][TN_];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < TN_; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

  // loader geometry: a "unit" = one 16-B chunk of columns x 2 consecutive m rows (bf16) or 1 row (fp32)
  constexpr int RPU = (sizeof(T) == 2) ? 2 : 1;      // m rows per unit
  constexpr int A_UNITS = A_CH * (TBK / RPU);
  constexpr int B_UNITS = B_CH * (TBK / RPU);
  constexpr int A_IT = A_UNITS / NTHREADS;           // bf16: 16*32/256 = 2 ; fp32: 32*64/256 = 8
  constexpr int B_IT = (B_UNITS + NTHREADS - 1) / NTHREADS;

  // per-thread fixed column chunk for B (patch gather resolves the segment once)
  const int fr = lane & 15, fg = lane >> 4;
  float colsum_local[PC], colsum_local_b[PC];
#pragma unroll
  for (int e = 0; e < PC; ++e) { colsum_local[e] = 0.f; colsum_local_b[e] = 0.f; }

  u32x4 va[A_IT][RPU], vb[B_IT][RPU];
  auto gload = [&](int mt) {
#pragma unroll
    for (int it = 0; it < A_IT; ++it) {
      int u = tid + it * NTHREADS;
      int c = u % A_CH, pr = u / A_CH;
      int n1 = n1_0 + c * PC;
#pragma unroll
      for (int q = 0; q < RPU; ++q) {
        int m = mt + pr * RPU + q;
        u32x4 v = {0u, 0u, 0u, 0u};
        if (m < m_end && n1 < p.N1) v = *(const u32x4*)(Ag + rowmap_base(amap, m) * p.lda + n1);
        va[it][q] = v;
      }
    }
#pragma unroll
    for (int it = 0; it < B_IT; ++it) {
      int u = tid + it * NTHREADS;
      int c = u % B_CH, pr = u / B_CH;
      int n2 = n2_0 + c * PC;
      int seg_rows = 0, col = n2, seg = 0;
      if (bmap.mode != 0) {
        seg = n2 / bmap.c_seg;
        col = n2 - seg * bmap.c_seg;
        if (bmap.mode == 1) seg_rows = rowmap_seg(bmap, seg);
      }
#pragma unroll
      for (int q = 0; q < RPU; ++q) {
        int m = mt + pr * RPU + q;
        u32x4 v = {0u, 0u, 0u, 0u};
        bool ok = u < B_UNITS && m < m_end && n2 < p.N2;
        int off = seg_rows;
        if (bmap.mode == 2 && ok) {
          int y, x;
          rowmap_yx(bmap, m, y, x);
          ok = rowmap_nb(bmap, seg, y, x, off);
        }
        if (ok) v = *(const u32x4*)(Bg + (rowmap_base(bmap, m) + off) * p.ldb + col);
        vb[it][q] = v;
      }
    }
  };
  gload(m_begin);
  for (int mt = m_begin; mt < m_end; mt += TBK) {
    __syncthreads();          // previous tile's fragment reads are done
#pragma unroll
    for (int it = 0; it < A_IT; ++it) {
      int u = tid + it * NTHREADS;
      int c = u % A_CH, pr = u / A_CH;
      if constexpr (sizeof(T) == 2) {
        bf16x8 x0 = __builtin_bit_cast(bf16x8, va[it][0]), x1 = __builtin_bit_cast(bf16x8, va[it][1]);
#pragma unroll
        for (int e = 0; e < 8; ++e) {
          bf16x2 pk = {x0[e], x1[e]};
          *(bf16x2*)(sA + (c * 8 + e) * ROWB + tsw(c * 8 + e, pr) * 4) = pk;
          if (do_colsum) colsum_local[e] += (float)x0[e] + (float)x1[e];
        }
      } else {
        f32x4 x0 = __builtin_bit_cast(f32x4, va[it][0]);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          *(float*)(sA + (c * 4 + e) * ROWB + pr * 4) = x0[e];
          if (do_colsum) colsum_local[e] += x0[e];
        }
      }
    }
#pragma unroll
    for (int it = 0; it < B_IT; ++it) {
      int u = tid + it * NTHREADS;
      if (u >= B_UNITS) continue;
      int c = u % B_CH, pr = u / B_CH;
      if constexpr (sizeof(T) == 2) {
        bf16x8 x0 = __builtin_bit_cast(bf16x8, vb[it][0]), x1 = __builtin_bit_cast(bf16x8, vb[it][1]);
#pragma unroll
        for (int e = 0; e < 8; ++e) {
          bf16x2 pk = {x0[e], x1[e]};
          *(bf16x2*)(sB + (c * 8 + e) * ROWB + tsw(c * 8 + e, pr) * 4) = pk;
          if (do_colsum_b) colsum_local_b[e] += (float)x0[e] + (float)x1[e];
        }
      } else {
        f32x4 x0 = __builtin_bit_cast(f32x4, vb[it][0]);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          *(float*)(sB + (c * 4 + e) * ROWB + pr * 4) = x0[e];
          if (do_colsum_b) colsum_local_b[e] += x0[e];
        }
      }
    }
    __syncthreads();
    if (mt + TBK < m_end) gload(mt + TBK);       // next tile's HBM reads fly while this tile's MFMAs run
    // fragments: row = n1 (or n2) index, 8 consecutive m at offset 32*ks + 8*fg
#pragma unroll
    for (int ks = 0; ks < TBK / 32; ++ks) {
      u32x4 fa[4][2], fb[TN_][2];
      constexpr int EB = sizeof(T);
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int n = wm * 64 + i * 16 + fr;
        const char* ptr = (EB == 2) ? sA + n * ROWB + tsw(n, ks * 16 + fg * 4) * 4 : sA + n * ROWB + (ks * 32 + fg * 8) * EB;
        fa[i][0] = *(const u32x4*)ptr;
        fa[i][1] = (EB == 4) ? *(const u32x4*)(ptr + 16) : fa[i][0];
      }
#pragma unroll
      for (int j = 0; j < TN_; ++j) {
        const int n = wn * WN + j * 16 + fr;
        const char* ptr = (EB == 2) ? sB + n * ROWB + tsw(n, ks * 16 + fg * 4) * 4 : sB + n * ROWB + (ks * 32 + fg * 8) * EB;
        fb[j][0] = *(const u32x4*)ptr;
        fb[j][1] = (EB == 4) ? *(const u32x4*)(ptr + 16) : fb[j][0];
      }
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < TN_; ++j) mma16(acc[i][j], fa[i][0], fa[i][1], fb[j][0], fb[j][1], (T*)nullptr);
    }
  }

  if (do_colsum) {
    // every A unit of this thread has the same column chunk c (A_CH divides NTHREADS)
    int c = tid % A_CH;
#pragma unroll
    for (int e = 0; e < PC; ++e) atomicAdd(&s_colsum[c * PC + e], colsum_local[e]);
    __syncthreads();
    if (tid < BM && n1_0 + tid < p.N1) atomicAdd(&p.colsum_a[n1_0 + tid], s_colsum[tid]);
  }
  if (do_colsum_b) {                 // only one of colsum_a / colsum_b is used per call (host wrapper checks)
    if (B_IT * NTHREADS == B_UNITS || tid < B_UNITS) {
      int c = tid % B_CH;
#pragma unroll
      for (int e = 0; e < PC; ++e) atomicAdd(&s_colsum[c * PC + e], colsum_local_b[e]);
    }
    __syncthreads();
    if (tid < BN && n2_0 + tid < p.N2) atomicAdd(&p.colsum_b[n2_0 + tid], s_colsum[tid]);
  }
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < TN_; ++j)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        int n1 = n1_0 + wm * 64 + i * 16 + 4 * fg + r;
        int n2 = n2_0 + wn * WN + j * 16 + fr;
        if (n1 < p.N1 && n2 < p.N2) atomicAdd(p.trans_c ? &p.C[(long)n2 * p.ldc + n1] : &p.C[(long)n1 * p.ldc + tn_dst_col(p, n2)], acc[i][j][r]);
      }
}

// ------------------------------------------------------------------------------------------------ TN, bf16, LDS-DMA
// Same contract as gemm_tn_kernel<bf16,BN>, different data path: tiles stay in their natural [m][n] layout and are
// filled by global_load_lds_dwordx4 (no VGPR round trip, no ds_write: the 2-byte transposing stores of the kernel
// above cost as many LDS cycles as the MFMAs they feed); the MFMA fragments (8 consecutive m of one n per lane) come
// from two ds_read_b64_tr_b16 each.  LDS-DMA writes lane-linear (base + 16*lane), so the bank swizzle is applied to
// the SOURCE column chunk: LDS slot s of tile row m holds global 16-B chunk s ^ (h(m) << 1), h spreading the 8 rows a
// 32-lane read group touches (m..m+3 and m+8..m+11) over the eight 32-B bank windows.  Rows past m_end / columns past
// N / out-of-image 3x3 taps are zero-filled by the owning lane.  Two buffers, one barrier per 64-row tile.  Column sums
// (bias gradients) are one extra MFMA against an all-ones fragment, shared between the two waves of a tile row.
// DG (plain rows, one BMT x BN = C x C output tile): the same pass over A = dY also produces the Linear's INPUT gradient dX = dY W -- the 64-row
// A tile is read a second time from LDS, row-wise, as the A operand of a [64 x C] x [C x C] product against W^T fragments that stay in
// registers (wave w owns output columns [w C/4, (w + 1) C/4)); the result leaves through an LDS tile as whole 16-byte row pieces one
// iteration later (so that its stores are a tile time old when the next counted vmcnt wait sees them).
template <int BMT, int BN, int BMODE, int NS, bool DG = false>
__global__ __launch_bounds__(NTHREADS, 2) void gemm_tn_dma_kernel(mvlt_gemm_tn_args p, int m_per_split, int t1, int t2, int splits, bf16* part = nullptr) {
  using TA = DmaTile<BMT>;
  using TB = DmaTile<BN>;
  static_assert(!DG || (BMODE == 3 && BMT == BN), "dgrad rides on the plain-row single-tile kernels");
  constexpr int WM = BMT / 2, TM_ = WM / 16;             // wave tile rows: 64 (4 fragments) or 32 (2)
  constexpr int WN = BN / 2, TN_ = WN / 16;
  constexpr int STAGE = TA::BYTES + TB::BYTES;
  constexpr int LPT = TA::IT + TB::IT;                    // DMA instructions per thread per tile
  extern __shared__ __attribute__((aligned(16))) char smem[];     // [NS][A tile | B tile]

  // XCD-aware order: workgroup b runs on XCD b % 8.  All t1*t2 output tiles of one m-split read the same rows of A
  // and B, so a whole split is given to ONE XCD (its tiles are consecutive in that XCD's queue and co-resident) and
  // the operands come through that XCD's L2 once instead of once per tile.
  // With fewer than 8 splits (M small, many output tiles: the vocabulary decoder) the natural order is kept instead:
  // x fastest, so the tiles sharing an A column slab (same x) meet on XCD x % 8.
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

  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm = wave >> 1, wn = wave & 1;
  const int n1_0 = bx * BMT, n2_0 = by * BN;
  const unsigned smem_lds = (unsigned)(uintptr_t)smem;      // LDS byte address of the dynamic segment
  const int m_begin = bz * m_per_split;
  const int m_end = min(p.M, m_begin + m_per_split);
  const RowMap amap = to_rowmap(p.a_map), bmap = to_rowmap(p.b_map);
  // bias gradients: every tile row (column) of workgroups sees the same A (B) rows; the t2 (t1) workgroups that share
  // them take turns, one 64-row tile each, so the extra MFMAs are spread evenly over the launch
  const bool do_colsum = p.colsum_a != nullptr;
  const bool do_colsum_b = p.colsum_b != nullptr;

  // ---- loader geometry (fixed per thread): LDS slot -> source column chunk
  const int a_row0 = tid / TA::CH;                                        // + RPP * j
  const int a_col = n1_0 + ((((tid % TA::CH)) ^ (TA::h(a_row0) << 1)) << 3);
  const bool a_col_ok = a_col < p.N1;
  const int b_row0 = tid / TB::CH;
  const int b_colg = n2_0 + ((((tid % TB::CH)) ^ (TB::h(b_row0) << 1)) << 3);
  const bool b_col_ok = b_colg < p.N2;
  int b_col = b_colg, b_seg_rows = 0, tap_dy = 0, tap_dx = 0;
  if constexpr (BMODE == 1 || BMODE == 2) {
    const int b_seg = b_colg / bmap.c_seg;
    b_col = b_colg - b_seg * bmap.c_seg;
    if constexpr (BMODE == 1) b_seg_rows = rowmap_seg(bmap, b_seg);
    else { tap_dy = b_seg / 3 - 1; tap_dx = b_seg - (b_seg / 3) * 3 - 1; }
  }
  const char* zsrc = (const char*)g_zero_page + ((tid * 16 + (blockIdx.x & 15) * 4096) & 65535);
  const char* a_src = (const char*)p.A + 2 * a_col;            // + physical row * row bytes
  const char* b_src = (const char*)p.B + 2 * b_col;
  const unsigned a_rowb = 2u * (unsigned)p.lda, b_rowb = 2u * (unsigned)p.ldb;
  const RowStep astep = row_step(amap, TBK), bstep = row_step(bmap, TBK);
  RowIt ait[TA::IT], bit[TB::IT];
#pragma unroll
  for (int j = 0; j < TA::IT; ++j) ait[j] = row_init(amap, m_begin + j * TA::RPP + a_row0);
#pragma unroll
  for (int j = 0; j < TB::IT; ++j) bit[j] = row_init(bmap, m_begin + j * TB::RPP + b_row0);

  // BMODE 3 = both operands with identity rows (most weight gradients): the source of a slot is a pointer that advances
  // by 64 rows per tile, and only the last (partial) tile of a split looks at row indices at all
  constexpr bool PLAIN = (BMODE == 3);
  const char* a_ptr[TA::IT];
  const char* b_ptr[TB::IT];
  const long a_adv = a_col_ok ? (long)TBK * a_rowb : 0, b_adv = b_col_ok ? (long)TBK * b_rowb : 0;
  if constexpr (PLAIN) {
#pragma unroll
    for (int j = 0; j < TA::IT; ++j) a_ptr[j] = a_col_ok ? a_src + (unsigned long long)(unsigned)(m_begin + j * TA::RPP + a_row0) * a_rowb : zsrc;
#pragma unroll
    for (int j = 0; j < TB::IT; ++j) b_ptr[j] = b_col_ok ? b_src + (unsigned long long)(unsigned)(m_begin + j * TB::RPP + b_row0) * b_rowb : zsrc;
  }
  // tiles are issued in order m_begin, m_begin + 64, ... (the row iterators advance by one tile per call)
  auto issue = [&](int mt, int slot) {
    if constexpr (PLAIN) {
      const bool whole = mt + TBK <= m_end;               // uniform
#pragma unroll
      for (int j = 0; j < TA::IT; ++j) {
        const int woff = slot * STAGE + (j * NTHREADS + wave * 64) * 16;
        const char* src = (whole || mt + j * TA::RPP + a_row0 < m_end) ? a_ptr[j] : zsrc;
        glds16(src, __builtin_amdgcn_readfirstlane(smem_lds + woff));
        a_ptr[j] += a_adv;
      }
#pragma unroll
      for (int j = 0; j < TB::IT; ++j) {
        const int woff = slot * STAGE + TA::BYTES + (j * NTHREADS + wave * 64) * 16;
        const char* src = (whole || mt + j * TB::RPP + b_row0 < m_end) ? b_ptr[j] : zsrc;
        glds16(src, __builtin_amdgcn_readfirstlane(smem_lds + woff));
        b_ptr[j] += b_adv;
      }
      return;
    }
#pragma unroll
    for (int j = 0; j < TA::IT; ++j) {
      int m = mt + j * TA::RPP + a_row0;
      int phys;
      bool ok = row_phys<0>(amap, ait[j], 0, 0, 0, phys) && m < m_end && a_col_ok;
      row_advance(ait[j], astep);
      const int woff = slot * STAGE + (j * NTHREADS + wave * 64) * 16;
      glds16(ok ? a_src + (unsigned long long)(unsigned)phys * a_rowb : zsrc, __builtin_amdgcn_readfirstlane(smem_lds + woff));
    }
#pragma unroll
    for (int j = 0; j < TB::IT; ++j) {
      int m = mt + j * TB::RPP + b_row0;
      int phys;
      bool ok = row_phys<(BMODE == 3 ? 0 : BMODE)>(bmap, bit[j], tap_dy, tap_dx, b_seg_rows, phys) && m < m_end && b_col_ok;
      row_advance(bit[j], bstep);
      const int woff = slot * STAGE + TA::BYTES + (j * NTHREADS + wave * 64) * 16;
      glds16(ok ? b_src + (unsigned long long)(unsigned)phys * b_rowb : zsrc, __builtin_amdgcn_readfirstlane(smem_lds + woff));
    }
  };

  // ---- fragment geometry: lane (g = lane>>4, L = lane&15) supplies tile row 8g + (L>>2), 8-B piece (L&3) of the
  //      16-column window of the n tile; second read 4 rows below; ks adds 32 rows
  const int g = lane >> 4, L = lane & 15;
  const int frow = 8 * g + (L >> 2);
  int aoff[TM_], boff[TN_];
#pragma unroll
  for (int i = 0; i < TM_; ++i) aoff[i] = TA::frag_off(frow, wm * TM_ + i, L);
#pragma unroll
  for (int j = 0; j < TN_; ++j) boff[j] = TB::frag_off(frow, wn * TN_ + j, L);

  f32x4 acc[TM_][TN_];
#pragma unroll
  for (int i = 0; i < TM_; ++i)
#pragma unroll
    for (int j = 0; j < TN_; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
  f32x4 cs[2] = {f32x4{0.f, 0.f, 0.f, 0.f}, f32x4{0.f, 0.f, 0.f, 0.f}};
  const u32x4 ones = {0x3F803F80u, 0x3F803F80u, 0x3F803F80u, 0x3F803F80u};
  bf16* const nb = nullptr;
  // ---- DG: W^T fragments of this wave's output columns (B operand: row n = input feature, 8 consecutive k = output features)
  constexpr int DGN = DG ? BN / 64 : 1, DGK = BMT / 32;
  u32x4 wtf[DGN][DGK];
  bf16* const sdX = (bf16*)(smem + NS * STAGE);              // [64][BN] parked dgrad tile
  if constexpr (DG) {
#pragma unroll
    for (int jn = 0; jn < DGN; ++jn)
#pragma unroll
      for (int ks = 0; ks < DGK; ++ks)
        wtf[jn][ks] = *(const u32x4*)((const bf16*)p.dgrad_wt + (long)((wave * DGN + jn) * 16 + (lane & 15)) * BMT + ks * 32 + (lane >> 4) * 8);
  }
  auto dg_store = [&](int mt_prev) {                         // the parked tile of rows mt_prev .. mt_prev + 63 -> dgrad_out, 16 bytes per thread and pass
    constexpr int CPR = BN / 8;
#pragma unroll
    for (int u = tid; u < 64 * CPR; u += NTHREADS) {
      const int r = u / CPR, c = u - r * CPR;
      if (mt_prev + r < m_end) *(u32x4*)((bf16*)p.dgrad_out + (long)(mt_prev + r) * p.dgrad_ld + c * 8) = *(const u32x4*)(sdX + r * BN + c * 8);
    }
  };

  // NS-deep ring: tile t+NS-1 is issued while tile t is consumed; the wait leaves the NS-2 younger tiles in flight.
  // Near the end fewer tiles are in flight than the count assumes, so the wait falls back to vmcnt(0) there; nothing
  // is issued past the last tile, so no DMA is outstanding when the epilogue reuses the LDS.
  // (Early slot release as in gemm_nt_dma_kernel -- every fragment read up front, a second barrier, the refill in front of the MFMAs -- was measured
  // slower here: 32 more registers to hold a whole tile's fragments, docs/experiments_r1-r3.md.)
#pragma unroll
  for (int st = 0; st < NS - 1; ++st)
    if (m_begin + st * TBK < m_end) issue(m_begin + st * TBK, st);
  int slot = 0, islot = NS - 1;
  for (int mt = m_begin; mt < m_end; mt += TBK) {
    constexpr int YOUNG = NS - 2;                        // younger tiles that may still be in flight when tile `mt` is needed
    if (YOUNG > 0 && mt + YOUNG * TBK < m_end) asm volatile("s_waitcnt vmcnt(%0) lgkmcnt(0)" ::"n"(LPT * (YOUNG > 0 ? YOUNG : 1)) : "memory");
    else asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();    // tile `mt` has landed for every wave; everyone is done reading the slot refilled next
    asm volatile("" ::: "memory");
    if constexpr (DG) { if (mt > m_begin) dg_store(mt - TBK); }      // (parked by every wave before this barrier)
    if (mt + (NS - 1) * TBK < m_end) issue(mt + (NS - 1) * TBK, islot);
    islot = islot + 1 == NS ? 0 : islot + 1;
    const char* sA = smem + slot * STAGE;
    const char* sB = sA + TA::BYTES;
    slot = slot + 1 == NS ? 0 : slot + 1;
    const int cs_turn = ((mt - m_begin) / TBK) % (do_colsum ? t2 : t1);
#pragma unroll
    for (int ks = 0; ks < TBK / 32; ++ks) {
      u32x4 fa[TM_], fb[TN_];
#pragma unroll
      for (int i = 0; i < TM_; ++i) fa[i] = tr_frag(sA + aoff[i] + ks * 32 * TA::ROWB, TA::ROWB);
#pragma unroll
      for (int j = 0; j < TN_; ++j) fb[j] = tr_frag(sB + boff[j] + ks * 32 * TB::ROWB, TB::ROWB);
#pragma unroll
      for (int i = 0; i < TM_; ++i)
#pragma unroll
        for (int j = 0; j < TN_; ++j) mma16(acc[i][j], fa[i], fa[i], fb[j], fb[j], nb);
      // column sums: the TM_ (TN_) fragments of a tile row (column) are shared by two waves; each takes half of them
      if (do_colsum && cs_turn == by) {
#pragma unroll
        for (int t = 0; t < TM_ / 2; ++t) {
          if (wn == 0) mma16(cs[t], fa[t], fa[t], ones, ones, nb);
          else mma16(cs[t], fa[TM_ / 2 + t], fa[TM_ / 2 + t], ones, ones, nb);
        }
      }
      if (do_colsum_b && cs_turn == bx) {
#pragma unroll
        for (int t = 0; t < TN_ / 2; ++t) {
          if (wm == 0) mma16(cs[t], ones, ones, fb[t], fb[t], nb);
          else mma16(cs[t], ones, ones, fb[TN_ / 2 + t], fb[TN_ / 2 + t], nb);
        }
      }
    }
    if constexpr (DG) {
      // dX tile [64 rows][BN]: row-wise A fragments of the dY tile (slot c of row r holds source chunk c ^ (h(r) << 1): an involution)
      const int dfr = lane & 15, dfg = lane >> 4;
      f32x4 dacc[4][DGN];
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int jn = 0; jn < DGN; ++jn) dacc[i][jn] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int ks = 0; ks < DGK; ++ks)
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const int row = i * 16 + dfr;
          const u32x4 af = *(const u32x4*)(sA + row * TA::ROWB + (((ks * 4 + dfg) ^ (TA::h(row) << 1)) << 4));
#pragma unroll
          for (int jn = 0; jn < DGN; ++jn) mma16(dacc[i][jn], af, af, wtf[jn][ks], wtf[jn][ks], nb);
        }
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
      __builtin_amdgcn_s_barrier();      // every thread has read the previous parked tile (its store-out sits in front of this iteration's MFMAs)
      asm volatile("" ::: "memory");
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int jn = 0; jn < DGN; ++jn)
#pragma unroll
          for (int r = 0; r < 4; ++r) sdX[(i * 16 + 4 * dfg + r) * BN + (wave * DGN + jn) * 16 + dfr] = (bf16)dacc[i][jn][r];
    }
  }
  if constexpr (DG) {
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __syncthreads();
    if (m_end > m_begin) dg_store(m_begin + ((m_end - m_begin - 1) / TBK) * TBK);
    __syncthreads();                     // (the column sums below reuse the front of the LDS)
  }

  const int fr = lane & 15, fg = lane >> 4;
  // column sums leave through LDS so that a workgroup sends one 64-lane atomic per 64 columns: every workgroup of the
  // launch adds into the same few cache lines, and those requests serialise at the memory side
  if (do_colsum || do_colsum_b) {
    float* s_cs = (float*)smem;
    __syncthreads();                 // all tile reads are done (uniform branch: by / bx are per workgroup)
    if (do_colsum && fr == 0) {      // cs[t][r]: tile row (wn*TM_/2+t)*16 + 4*fg + r, identical in every lane column
#pragma unroll
      for (int t = 0; t < TM_ / 2; ++t)
#pragma unroll
        for (int r = 0; r < 4; ++r) s_cs[wm * WM + (wn * (TM_ / 2) + t) * 16 + 4 * fg + r] = cs[t][r];
    }
    if (do_colsum_b && fg == 0) {    // cs[t][0]: tile column (wm*TN_/2+t)*16 + fr
#pragma unroll
      for (int t = 0; t < TN_ / 2; ++t) s_cs[wn * WN + (wm * (TN_ / 2) + t) * 16 + fr] = cs[t][0];
    }
    __syncthreads();
    if (do_colsum && tid < BMT && n1_0 + tid < p.N1) atomicAdd(&p.colsum_a[n1_0 + tid], s_cs[tid]);
    if (do_colsum_b && tid < BN && n2_0 + tid < p.N2) atomicAdd(&p.colsum_b[n2_0 + tid], s_cs[tid]);
  }
  if (part) {
    // PARTIAL-TILE mode (round 5; the host chooses it for outputs that many m-splits meet on: the q / proj weight gradients of stages 3-4 spent 14-21 us of 53-56 us in
    // 5.7-8.4 M fp32 atomics): this split's tile goes to part[split][N1][N2] in bf16 -- 16 rows at a time through a per-wave LDS tile, out as 16-byte pieces of contiguous
    // rows -- and tn_fold_kernel adds the splits in order (deterministic).  N2 % 8 == 0 (host), rows past N1 and 8-column pieces past N2 are not stored.
    constexpr int LDP = WN + 8;
    __syncthreads();                                    // every wave is done with the operand tiles (and the column sums) this overlays
    bf16* const st = (bf16*)smem + wave * 16 * LDP;
    bf16* const P = part + (size_t)bz * p.N1 * p.N2;
#pragma unroll
    for (int i = 0; i < TM_; ++i) {
      __builtin_amdgcn_wave_barrier();
#pragma unroll
      for (int j = 0; j < TN_; ++j)
#pragma unroll
        for (int r = 0; r < 4; ++r) st[(4 * fg + r) * LDP + j * 16 + fr] = (bf16)acc[i][j][r];
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
      __builtin_amdgcn_wave_barrier();
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
#pragma unroll
      for (int q = lane; q < 16 * (WN / 8); q += 64) {
        const int row = q / (WN / 8), ch = q - row * (WN / 8);
        const int n1 = n1_0 + wm * WM + i * 16 + row, n2 = n2_0 + wn * WN + ch * 8;
        if (n1 < p.N1 && n2 < p.N2) st_g<MVLT_NT_GEMM>((u32x4*)(P + (size_t)n1 * p.N2 + n2), *(const u32x4*)(st + row * LDP + ch * 8));
      }
    }
    return;
  }
  if (p.c_overwrite) {
    // round 6: C = (not +=) this launch's single m-split (the caller vouches for a zeroed C: the vocabulary decoder's weight gradient, 30522 x 768 = 23 M outputs whose
    // fire-and-forget fp32 atomics were most of the launch).  16 rows of the wave tile at a time through a per-wave LDS tile, out as 16-byte pieces of contiguous rows.
    constexpr int LDP = WN + 4;
    constexpr int CPR = WN / 4;
    __syncthreads();                                   // every wave is done with the operand tiles this overlays
    float* const st = (float*)smem + wave * 16 * LDP;
#pragma unroll
    for (int i = 0; i < TM_; ++i) {
      __builtin_amdgcn_wave_barrier();
#pragma unroll
      for (int j = 0; j < TN_; ++j)
#pragma unroll
        for (int r = 0; r < 4; ++r) st[(4 * fg + r) * LDP + j * 16 + fr] = acc[i][j][r];
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
      __builtin_amdgcn_wave_barrier();
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
#pragma unroll
      for (int q = lane; q < 16 * CPR; q += 64) {
        const int row = q / CPR, ch = q - row * CPR;
        const int n1 = n1_0 + wm * WM + i * 16 + row, n2 = n2_0 + wn * WN + ch * 4;
        if (n1 < p.N1 && n2 < p.N2) st_g<MVLT_NT_GEMM>((f32x4*)(p.C + (size_t)n1 * p.ldc + n2), *(const f32x4*)(st + row * LDP + ch * 4));
      }
    }
    return;
  }
#pragma unroll
  for (int i = 0; i < TM_; ++i)
#pragma unroll
    for (int j = 0; j < TN_; ++j)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        int n1 = n1_0 + wm * WM + i * 16 + 4 * fg + r;
        int n2 = n2_0 + wn * WN + j * 16 + fr;
        if (n1 < p.N1 && n2 < p.N2) atomicAdd(p.trans_c ? &p.C[(long)n2 * p.ldc + n1] : &p.C[(long)n1 * p.ldc + tn_dst_col(p, n2)], acc[i][j][r]);
      }
}

}  // namespace

// ------------------------------------------------------------------------------------------------ plan -> launch
int mvlt_launch_tn_dma(const mvlt_gemm_plan& p, const mvlt_gemm_tn_args& k, bf16* part, hipStream_t s) {
  const char* const who = "mvlt_gemm_tn";
  MVLT_PLAN_LAUNCH_HEAD;
#define TN_PLAIN(T_, DT_, BN_) MVLT_CASE(false, (gemm_tn_kernel<T_, BN_>), (MVLT_GEMM_TN_PLAIN, DT_, BN_), k, p.per_split)
#define TN_DMA(BMT_, BN_, BMODE_, NS_, DG_) \
  MVLT_CASE(DG_, (gemm_tn_dma_kernel<BMT_, BN_, BMODE_, NS_, DG_>), (MVLT_GEMM_TN_DMA, BMT_, BN_, BMODE_, NS_, DG_), k, p.per_split, p.t1, p.t2, p.splits, part)
#define TN_DMA_MODES(BMT_, BN_, NS_) TN_DMA(BMT_, BN_, 3, NS_, false) TN_DMA(BMT_, BN_, 0, NS_, false) TN_DMA(BMT_, BN_, 1, NS_, false) TN_DMA(BMT_, BN_, 2, NS_, false)
  switch (key) {
    TN_DMA(64, 64, 3, 4, true) TN_DMA(128, 128, 3, 2, true)
    TN_DMA_MODES(128, 128, 2) TN_DMA_MODES(128, 64, 3) TN_DMA_MODES(64, 128, 3) TN_DMA_MODES(64, 64, 4)
    TN_PLAIN(bf16, 0, 64) TN_PLAIN(bf16, 0, 128) TN_PLAIN(float, 1, 64) TN_PLAIN(float, 1, 128)
  }
  return no_instantiation(who, p);
}

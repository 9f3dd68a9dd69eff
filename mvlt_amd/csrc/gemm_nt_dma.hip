// NT GEMM, 4 waves, 128 x BN tiles: the register-staged kernel (the fp32 path) and the bf16 LDS-DMA kernel.  Overview: gemm.hip.
#include "gemm_common.h"

namespace {

// ------------------------------------------------------------------------------------------------ NT
template <typename T, int BN>
__global__ __launch_bounds__(NTHREADS) void gemm_nt_kernel(mvlt_gemm_nt_args p, int nbuf) {
  constexpr int BK = Elem<T>::BK;
  constexpr int PC = Elem<T>::PER_CHUNK;
  constexpr int WN = BN / 2;            // wave tile N
  constexpr int TN_ = WN / 16;          // 16-wide MFMA tiles per wave in N
  constexpr int A_ITERS = BM * CHUNKS / NTHREADS;   // 4
  constexpr int B_ITERS = BN * CHUNKS / NTHREADS;   // 4 or 2
  extern __shared__ __attribute__((aligned(16))) char smem[];
  char* sA = smem;                                   // nbuf x BM x 128 B  (nbuf = 1 when K fits one tile: 2x the
  char* sB = smem + nbuf * BM * ROW_BYTES;           // nbuf x BN x 128 B   workgroups per CU for the K=64 stage-1 GEMMs)

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave >> 1, wn = wave & 1;
  // XCD-aware order (block b runs on XCD b % 8): the column tiles of one 128-row panel get consecutive slots on ONE XCD,
  // so the A panel is fetched into that XCD's L2 once and a row block of C is written as a whole (all its column tiles
  // close together in time) instead of as 256-byte slivers revisited tiles_m workgroups later.
  const int tiles_m = (p.M + BM - 1) / BM;
  const int tiles_n = (p.N + BN - 1) / BN;
  const int bid = blockIdx.x;
  const int xcd = bid & 7, slot = bid >> 3;
  const int tile_m = (slot / tiles_n) * 8 + xcd, tile_n = slot % tiles_n;
  if (tile_m >= tiles_m) return;
  const int m0 = tile_m * BM, n0 = tile_n * BN;
  const RowMap amap = to_rowmap(p.a_map);

  const int chunk = tid & 7;
  const int row_in = tid >> 3;          // 0..31
  const T* Ag = (const T*)p.A;
  const T* Bg = (const T*)p.B;

  long a_base[A_ITERS];
  bool a_ok[A_ITERS];
  int a_y[A_ITERS], a_x[A_ITERS];       // mode 2 only: pixel coordinates (zero-padding test per 3x3 tap)
#pragma unroll
  for (int i = 0; i < A_ITERS; ++i) {
    int m = m0 + row_in + 32 * i;
    a_ok[i] = m < p.M;
    a_base[i] = a_ok[i] ? rowmap_base(amap, m) : 0;
    a_y[i] = 0; a_x[i] = 0;
    if (amap.mode == 2 && a_ok[i]) rowmap_yx(amap, m, a_y[i], a_x[i]);
  }
  long b_base[B_ITERS];
  bool b_ok[B_ITERS];
#pragma unroll
  for (int i = 0; i < B_ITERS; ++i) {
    int n = n0 + row_in + 32 * i;
    b_ok[i] = n < p.N;
    b_base[i] = b_ok[i] ? (long)n * p.ldb : 0;
  }

  u32x4 ra[A_ITERS], rb[B_ITERS];
  auto gload = [&](int kt) {
    const int k = kt * BK + chunk * PC;
    const bool k_ok = k < p.K;          // K % PER_CHUNK == 0 is required by the host wrapper
    int seg_rows = 0, kk = k, seg = 0;
    if (amap.mode != 0) {
      seg = k / amap.c_seg;
      kk = k - seg * amap.c_seg;
      if (amap.mode == 1) seg_rows = rowmap_seg(amap, seg);
    }
#pragma unroll
    for (int i = 0; i < A_ITERS; ++i) {
      u32x4 v = {0u, 0u, 0u, 0u};
      bool ok = a_ok[i] && k_ok;
      int off = seg_rows;
      if (amap.mode == 2) ok = ok && rowmap_nb(amap, seg, a_y[i], a_x[i], off);
      if (ok) v = *(const u32x4*)(Ag + (a_base[i] + off) * p.lda + kk);
      ra[i] = v;
    }
#pragma unroll
    for (int i = 0; i < B_ITERS; ++i) {
      u32x4 v = {0u, 0u, 0u, 0u};
      if (b_ok[i] && k_ok) v = *(const u32x4*)(Bg + b_base[i] + k);
      rb[i] = v;
    }
  };
  auto lstore = [&](int buf) {
#pragma unroll
    for (int i = 0; i < A_ITERS; ++i) {
      int r = row_in + 32 * i;
      *(u32x4*)(sA + buf * BM * ROW_BYTES + r * ROW_BYTES + swz(r, chunk) * 16) = ra[i];
    }
#pragma unroll
    for (int i = 0; i < B_ITERS; ++i) {
      int r = row_in + 32 * i;
      *(u32x4*)(sB + buf * BN * ROW_BYTES + r * ROW_BYTES + swz(r, chunk) * 16) = rb[i];
    }
  };

  f32x4 acc[4][TN_];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < TN_; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

  const int nk = (p.K + BK - 1) / BK;
  gload(0);
  lstore(0);
  __syncthreads();
  const int fr = lane & 15, fg = lane >> 4;
  for (int kt = 0; kt < nk; ++kt) {
    const int buf = kt & 1;
    if (kt + 1 < nk) gload(kt + 1);
    const char* a_s = sA + buf * BM * ROW_BYTES + (wm * 64) * ROW_BYTES;
    const char* b_s = sB + buf * BN * ROW_BYTES + (wn * WN) * ROW_BYTES;
    constexpr int KSTEPS = (sizeof(T) == 2) ? 2 : 1;     // k32 steps per LDS tile
    constexpr int CPS = (sizeof(T) == 2) ? 1 : 2;        // 16-B chunks per fragment
#pragma unroll
    for (int ks = 0; ks < KSTEPS; ++ks) {
      u32x4 fa[4][2], fb[TN_][2];
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        int r = i * 16 + fr;
        int rr = wm * 64 + r;           // swizzle uses the tile-level row
#pragma unroll
        for (int c = 0; c < CPS; ++c) {
          int ch = (sizeof(T) == 2) ? (ks * 4 + fg) : (fg * 2 + c);
          fa[i][c] = *(const u32x4*)(a_s + r * ROW_BYTES + swz(rr, ch) * 16);
        }
        if (CPS == 1) fa[i][1] = fa[i][0];
      }
#pragma unroll
      for (int j = 0; j < TN_; ++j) {
        int r = j * 16 + fr;
        int rr = wn * WN + r;
#pragma unroll
        for (int c = 0; c < CPS; ++c) {
          int ch = (sizeof(T) == 2) ? (ks * 4 + fg) : (fg * 2 + c);
          fb[j][c] = *(const u32x4*)(b_s + r * ROW_BYTES + swz(rr, ch) * 16);
        }
        if (CPS == 1) fb[j][1] = fb[j][0];
      }
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < TN_; ++j) mma16(acc[i][j], fa[i][0], fa[i][1], fb[j][0], fb[j][1], (T*)nullptr);
    }
    if (kt + 1 < nk) lstore(buf ^ 1);
    __syncthreads();
  }

  nt_epilogue<T, BN>(p, acc, smem, m0, n0, wave, lane);
}

// ------------------------------------------------------------------------------------------------ NT, bf16, LDS-DMA
// gemm_nt_kernel<bf16,BN> with the operand tiles filled by global_load_lds_dwordx4 instead of load -> VGPR ->
// ds_write_b128 (LDS stores run at ~80 B/clk/CU, a third of the read rate, and were as expensive as the MFMAs).  The
// LDS image is the same (128-B rows of 64 k, 16-B chunks XOR-swizzled by row); because the DMA writes lane-linear the
// swizzle is applied to the source chunk each lane fetches.  ns-deep ring with a counted vmcnt wait, as in the TN kernel.
template <int BN, int AMODE, int EPI, int BK, int BMT = BM>
__global__ __launch_bounds__(NTHREADS, BMT == 256 ? 2 : 1) void gemm_nt_dma_kernel(mvlt_gemm_nt_args p, int ns_flags) {
  const int ns = ns_flags & 0xff;                   // ring depth
  const bool early = (ns_flags & 0x100) != 0;       // early slot release (below)
  constexpr int ROWB = BK * 2;                      // LDS row: BK k-values of one tile row
  constexpr int CH = BK / 8;                        // 16-B chunks per row (8 or 4)
  constexpr int RPL = NTHREADS / CH;                // tile rows one DMA instruction of the workgroup covers
  constexpr int WN = BN / 2, TN_ = WN / 16;
  // BMT = 256 (wave tile 128 x 64 with 32-wide K stages, a quarter less operand traffic per MFMA) was measured and is not
  // dispatched: -5 % on 49152x2048x512 and the 256-channel conv shape, +13 % on 98304x320x1280, worse under every R / H epilogue
  constexpr int WM = BMT / 2, TM_ = WM / 16;        // wave tile rows: 64
  constexpr int A_ITERS = BMT * CH / NTHREADS;      // 4 (BK 64) or 2 (BK 32) at 128 rows
  constexpr int B_ITERS = BN * CH / NTHREADS;
  constexpr int LPT = A_ITERS + B_ITERS;
  constexpr int STAGE = (BMT + BN) * ROWB;
  // chunk swizzle by row: 16 consecutive rows x one logical chunk must spread over all 64 banks
  // (four chunks per row, BK = 32: a ds_read_b128 lane group holds rows {r, r+12} at one chunk and {r+4, r+8} at the next for each r & 3 --
  // the mask must differ between those four row quads in a way that keeps chunk ^ mask distinct: (-(row >> 2)) & 3 does, (row >> 2) & 3, round
  // 2's choice, maps them onto two slots: 43 % LDS bank conflicts in the stage-3 fc1 + GELU launch)
  auto swzk = [](int row, int chunk) { return CH == 8 ? (chunk ^ ((row >> 1) & 7)) : (chunk ^ ((0 - (row >> 2)) & 3)); };
  extern __shared__ __attribute__((aligned(16))) char smem[];

  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm = wave >> 1, wn = wave & 1;
  const int tiles_m = (p.M + BMT - 1) / BMT;
  const int tiles_n = (p.N + BN - 1) / BN;
  const int bid = blockIdx.x;
  const int xcd = bid & 7, bslot = bid >> 3;
  const int tile_m = (bslot / tiles_n) * 8 + xcd, tile_n = bslot % tiles_n;
  if (tile_m >= tiles_m) return;
  const int m0 = tile_m * BMT, n0 = tile_n * BN;
  const RowMap amap = to_rowmap(p.a_map);
  const unsigned smem_lds = (unsigned)(uintptr_t)smem;

  const int row_in = tid / CH;                                  // 0..RPL-1 (+RPL i)
  const int chunk = swzk(row_in, tid % CH);                     // source chunk of this thread's LDS slot: swz is an involution
  const char* zsrc = (const char*)g_zero_page + ((tid * 16 + (bid & 15) * 4096) & 65535);

  const char* a_ptr[A_ITERS];
  bool a_ok[A_ITERS];
  int a_y[A_ITERS], a_x[A_ITERS];
#pragma unroll
  for (int i = 0; i < A_ITERS; ++i) {
    int m = m0 + row_in + RPL * i;
    a_ok[i] = m < p.M;
    RowIt it = row_init(amap, a_ok[i] ? m : 0);
    int phys;
    if constexpr (AMODE == 0) phys = it.b * amap.batch_stride + amap.offset + it.x;
    else if constexpr (AMODE == 1) phys = it.b * amap.tokens_in + (it.y * amap.r) * amap.w_in + it.x * amap.r;
    else phys = it.b * amap.tokens_in + it.y * amap.w_in + it.x;                   // centre pixel
    a_y[i] = it.y; a_x[i] = it.x;
    a_ptr[i] = (const char*)p.A + (unsigned long long)(unsigned)phys * (2u * (unsigned)p.lda);
  }
  const char* b_ptr[B_ITERS];
  bool b_ok[B_ITERS];
#pragma unroll
  for (int i = 0; i < B_ITERS; ++i) {
    int n = n0 + row_in + RPL * i;
    b_ok[i] = n < p.N;
    b_ptr[i] = (const char*)p.B + (unsigned long long)(unsigned)(b_ok[i] ? n : 0) * (2u * (unsigned)p.ldb);
  }

  // K position of this thread's chunk, kept as (segment, offset in segment) for the gather maps; advanced per tile
  // K split (blockIdx.y): this workgroup reduces k-tiles [kt0, kt0 + nk) and adds its partial tile atomically
  const int nk_all = (p.K + BK - 1) / BK;
  const int nsplit = p.split_k > 1 ? p.split_k : 1;
  const int kt_per = (nk_all + nsplit - 1) / nsplit;
  const int kt0 = blockIdx.y * kt_per;
  int kpos = kt0 * BK + chunk * 8, seg = 0, kk = kpos;                   // (a K split of a gathered A starts inside a later segment)
  if constexpr (AMODE != 0) { seg = kk / amap.c_seg; kk -= seg * amap.c_seg; }
  auto issue = [&](int slot) {                                  // tiles are issued in K order
    const bool k_ok = kpos < p.K;
    int off_bytes = (AMODE == 0 ? kpos : kk) * 2, tdy = 0, tdx = 0;
    if constexpr (AMODE == 1) off_bytes += rowmap_seg(amap, seg) * (2 * p.lda);
    if constexpr (AMODE == 2) {
      const int dy = seg / 3;
      tdy = dy - 1; tdx = seg - dy * 3 - 1;
      off_bytes += (tdy * amap.w_in + tdx) * (2 * p.lda);
    }
#pragma unroll
    for (int i = 0; i < A_ITERS; ++i) {
      bool ok = a_ok[i] && k_ok;
      if constexpr (AMODE == 2) ok = ok && (unsigned)(a_y[i] + tdy) < (unsigned)amap.h_in && (unsigned)(a_x[i] + tdx) < (unsigned)amap.w_in;
      glds16(ok ? a_ptr[i] + off_bytes : zsrc, __builtin_amdgcn_readfirstlane(smem_lds + slot * STAGE + (i * NTHREADS + wave * 64) * 16));
    }
#pragma unroll
    for (int i = 0; i < B_ITERS; ++i)
      glds16((b_ok[i] && k_ok) ? b_ptr[i] + kpos * 2 : zsrc,
             __builtin_amdgcn_readfirstlane(smem_lds + slot * STAGE + BMT * ROWB + (i * NTHREADS + wave * 64) * 16));
    kpos += BK;
    if constexpr (AMODE != 0) {
      kk += BK;
      while (kk >= amap.c_seg) { kk -= amap.c_seg; ++seg; }
    }
  };

  f32x4 acc[TM_][TN_];
#pragma unroll
  for (int i = 0; i < TM_; ++i)
#pragma unroll
    for (int j = 0; j < TN_; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

  const int nk = min(kt_per, nk_all - kt0);
  if (nk <= 0) return;
  const int fr = lane & 15, fg = lane >> 4;
  // Early slot release: every fragment of a stage is read into registers before its first MFMA, so the stage's slot is free as soon as all
  // four waves have done those reads -- a second barrier right behind them -- and the refill (stage kt + ns) is issued THERE, in front of
  // the MFMAs, instead of behind the barrier of the next k-step: ns stages in flight per workgroup instead of ns - 1.  With the
  // two-slot ring the K-loop otherwise runs at one LDS-DMA latency per k-step (Little's law with the LDS as the window).
  for (int st = 0; st < (early ? ns : ns - 1) && st < nk; ++st) issue(st);
  if (ns == 1 && !early) issue(0);
  int slot = 0, islot = early ? 0 : ns - 1;
  for (int kt = 0; kt < nk; ++kt) {
    // tile kt must have landed; up to ns - 2 (early: ns - 1) later tiles may still be in flight (none near the tail)
    const int ahead = min(nk - 1 - kt, early ? ns - 1 : ns - 2);
    if (ahead >= 4) asm volatile("s_waitcnt vmcnt(%0) lgkmcnt(0)" ::"n"(4 * LPT) : "memory");
    else if (ahead == 3) asm volatile("s_waitcnt vmcnt(%0) lgkmcnt(0)" ::"n"(3 * LPT) : "memory");
    else if (ahead == 2) asm volatile("s_waitcnt vmcnt(%0) lgkmcnt(0)" ::"n"(2 * LPT) : "memory");
    else if (ahead == 1) asm volatile("s_waitcnt vmcnt(%0) lgkmcnt(0)" ::"n"(LPT) : "memory");
    else asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    asm volatile("" ::: "memory");
    if (!early) {
      if (ns > 1 && kt + ns - 1 < nk) issue(islot);
      islot = islot + 1 >= ns ? 0 : islot + 1;
    }
    const char* a_s = smem + slot * STAGE + (wm * WM) * ROWB;
    const char* b_s = smem + slot * STAGE + BMT * ROWB + (wn * WN) * ROWB;
    slot = slot + 1 >= ns ? 0 : slot + 1;
    // every fragment of the tile is requested before the first MFMA (both 32-k halves): the compiler otherwise recycles one
    // fragment set and waits out the LDS latency three times per half
    constexpr int KS = BK / 32;
    u32x4 fa[KS][TM_], fb[KS][TN_];
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) {
#pragma unroll
      for (int i = 0; i < TM_; ++i) {
        int r = i * 16 + fr;
        fa[ks][i] = *(const u32x4*)(a_s + r * ROWB + swzk(wm * WM + r, ks * 4 + fg) * 16);
      }
#pragma unroll
      for (int j = 0; j < TN_; ++j) {
        int r = j * 16 + fr;
        fb[ks][j] = *(const u32x4*)(b_s + r * ROWB + swzk(wn * WN + r, ks * 4 + fg) * 16);
      }
    }
    if (early) {
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
      __builtin_amdgcn_s_barrier();                  // every wave holds its fragments of stage kt: the slot may be refilled
      asm volatile("" ::: "memory");
      if (kt + ns < nk) issue(islot);
      islot = islot + 1 >= ns ? 0 : islot + 1;
    }
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) {
      __builtin_amdgcn_sched_barrier(0);             // keeps every ds_read ahead of the MFMAs (one wait per tile)
#pragma unroll
      for (int i = 0; i < TM_; ++i)
#pragma unroll
        for (int j = 0; j < TN_; ++j) mma16(acc[i][j], fa[ks][i], fa[ks][i], fb[ks][j], fb[ks][j], (bf16*)nullptr);
    }
  }
  __syncthreads();                   // last tile's reads are done before the epilogue reuses the LDS
  static_assert(BMT == BM || (BN != 192 && EPI != 0), "the 256-row tile carries the lean epilogues only");
  if constexpr (BN == 192) nt_epilogue_192<EPI>(p, acc, smem, m0, n0, wave, lane);
  else if constexpr (EPI == 0) nt_epilogue<bf16, BN>(p, acc, smem, m0, n0, wave, lane);
  else nt_epilogue_lean<BN, EPI, TM_>(p, acc, smem, m0, n0, wave, lane);
}

}  // namespace

// ------------------------------------------------------------------------------------------------ plan -> launch
int mvlt_launch_nt_dma(const mvlt_gemm_plan& p, const mvlt_gemm_nt_args& a, hipStream_t s) {
  const char* const who = "mvlt_gemm_nt";
  MVLT_PLAN_LAUNCH_HEAD;
#define NT_F32(BN_) MVLT_CASE(false, (gemm_nt_kernel<float, BN_>), (MVLT_GEMM_NT_F32, BN_), a, p.nbuf)
#define NT_DMA(BN_, AM_, EPI_, BK_) MVLT_CASE(false, (gemm_nt_dma_kernel<BN_, AM_, EPI_, BK_>), (MVLT_GEMM_NT_DMA, BN_, AM_, EPI_, BK_), a, p.ns_flags)
#define NT_DMA_EPIS(BN_, AM_) NT_DMA(BN_, AM_, 1, 64) NT_DMA(BN_, AM_, 2, 64) NT_DMA(BN_, AM_, 3, 64) NT_DMA(BN_, AM_, 4, 64) \
                              NT_DMA(BN_, AM_, 5, 64) NT_DMA(BN_, AM_, 6, 64) NT_DMA(BN_, AM_, 7, 64) NT_DMA(BN_, AM_, 0, 64)
  switch (key) {
    NT_DMA(64, 0, 8, 64) NT_DMA(128, 0, 8, 64)
    NT_DMA(192, 0, 1, 64) NT_DMA(192, 0, 5, 64) NT_DMA(192, 2, 1, 64) NT_DMA(192, 2, 5, 64)
    NT_DMA_EPIS(64, 0) NT_DMA_EPIS(64, 1) NT_DMA_EPIS(64, 2)
    NT_DMA(128, 0, 3, 32) NT_DMA(128, 0, 4, 32)
    NT_DMA_EPIS(128, 0) NT_DMA_EPIS(128, 1) NT_DMA_EPIS(128, 2)
    NT_F32(64) NT_F32(128)
  }
  return no_instantiation(who, p);
}

// The MIM decoder's conv3x3 on an LDS halo: weight gradient (a TN launch) and forward / input gradient (an NT launch).  Overview: gemm.hip.
#include "gemm_common.h"

namespace {

// ------------------------------------------------------------------------------------------------ conv3x3 weight gradient, LDS halo
// dW[o][tap][c] += sum over pixels dz[pixel][o] * x[pixel + tap][c]: the weight gradient of the MIM decoder's conv3x3 (reference
// libs/vl_heads.py:116-129) on pixel-major data.  As the generic TN GEMM with the 3x3 gather on B (BMODE 2 above) every tap re-fetches
// its shifted copy of the input rows through the LDS-DMA path -- 9 x 64 rows of B per 64-pixel k-tile -- and that path, not the MFMAs,
// bounds the GEMM loops of this chip (round-2 ablations): 96 B/clk/CU asked of a path that sustains ~16-20.
// Here a workgroup owns a 64 (out) x 9 (taps) x 64 (in) block of dW in registers (36 accumulator tiles per wave) and, per k-tile of
// 64 pixels (= 64 / W whole image rows), loads the pixels' HALO once -- (64/W + 2) x (W + 2) input rows of 64 channels, 17 KB at
// W = 32 instead of 72 KB -- and forms all nine taps' B fragments from it by transposed LDS reads at shifted row addresses (pixels of
// a fragment are consecutive in one image row, so a tap is a constant row offset; out-of-image halo rows come from the zero page).
// 25 KB through the DMA path per 4.7 MFLOP: ~22 B/clk/CU at full MFMA rate.
template <int W>
__global__ __launch_bounds__(NTHREADS, 2) void conv3_wgrad_kernel(mvlt_gemm_tn_args p, int tiles_per_split, int n_o, int n_c, int splits, bf16* part) {
  using TA = DmaTile<64>;
  constexpr int R = 64 / W;                         // image rows per 64-pixel k-tile
  constexpr int HW2 = W + 2, HR = (R + 2) * HW2;    // halo rows (one pixel each, 64 channels = 128 B)
  constexpr int H_IT = (HR * 8 + NTHREADS - 1) / NTHREADS;          // DMA instructions per thread for the halo (last one partly idle)
  constexpr int HALO_BYTES = H_IT * NTHREADS * 16;
  constexpr int STAGE = TA::BYTES + HALO_BYTES;
  extern __shared__ __attribute__((aligned(16))) char smem[];      // [2][dz tile | halo tile]
  const int txy = n_o * n_c;
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
  const int bo = xy % n_o, bc = xy / n_o;
  const int o0 = bo * 64, c0 = bc * 64;
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm = wave >> 1, wn = wave & 1;
  const unsigned smem_lds = (unsigned)(uintptr_t)smem;
  const int ntiles = p.M / 64;
  const int t_begin = bz * tiles_per_split, t_end = min(ntiles, t_begin + tiles_per_split);
  const int Himg = p.b_map.h_in, cin = p.b_map.c_seg, tokens_in = p.b_map.tokens_in;
  const int tiles_per_img = Himg * W / 64;
  const char* zsrc = (const char*)g_zero_page + ((tid * 16 + (blockIdx.x & 15) * 4096) & 65535);

  // ---- loader geometry.  dz tile: as the TN kernel's A tile (64 pixels x 64 outputs, chunks swizzled by TA::h on the source side)
  const int a_row0 = tid / TA::CH;
  const int a_col = o0 + (((tid % TA::CH) ^ (TA::h(a_row0) << 1)) << 3);
  const char* a_src = (const char*)p.A + 2 * a_col;
  const unsigned a_rowb = 2u * (unsigned)p.lda, b_rowb = 2u * (unsigned)p.ldb;
  // halo tile: LDS row hr = (hy, hx) of the padded (R+2) x (W+2) window; slot s of row hr holds source chunk s ^ (hh(hr) << 1).
  // The bank hash of this tile uses bit 1 of the row only: a fragment's second read sits 4 rows below its first at ANY row
  // alignment here (taps shift the rows by +-1 and +-(W+2)), so the hash must not change under +4 (TA::h does when bit 2 is set).
  // Rows r..r+3 land on four distinct (bank half, window) pairs, the +8 group repeats them: 2-way conflicts, LDS stays off the
  // critical path (72 transposed reads per 36 MFMAs).
  auto hh = [](int row) { return (row >> 1) & 1; };
  int h_dy[H_IT], h_off[H_IT];
  bool h_xok[H_IT];
#pragma unroll
  for (int j = 0; j < H_IT; ++j) {
    const int q = tid + j * NTHREADS, hr = q >> 3, sl = q & 7;
    const int hy = hr / HW2, hx = hr - hy * HW2;
    h_dy[j] = hy - 1;
    h_xok[j] = hr < HR && (unsigned)(hx - 1) < (unsigned)W;
    h_off[j] = (hx - 1) * (int)b_rowb + 2 * (c0 + ((sl ^ (hh(hr) << 1)) << 3));
  }
  auto issue = [&](int tile, int slot) {
    const int img = tile / tiles_per_img, y0 = (tile - img * tiles_per_img) * R;
#pragma unroll
    for (int j = 0; j < TA::IT; ++j) {
      const unsigned m = (unsigned)(tile * 64 + j * TA::RPP + a_row0);
      glds16(a_src + (unsigned long long)m * a_rowb, __builtin_amdgcn_readfirstlane(smem_lds + slot * STAGE + (j * NTHREADS + wave * 64) * 16));
    }
    const char* img_base = (const char*)p.B + (unsigned long long)(unsigned)(img * tokens_in) * b_rowb;
#pragma unroll
    for (int j = 0; j < H_IT; ++j) {
      const int y = y0 + h_dy[j];
      const bool ok = h_xok[j] && (unsigned)y < (unsigned)Himg;
      glds16(ok ? img_base + (long)(y * W) * (long)b_rowb + h_off[j] : zsrc,
             __builtin_amdgcn_readfirstlane(smem_lds + slot * STAGE + TA::BYTES + (j * NTHREADS + wave * 64) * 16));
    }
  };

  // ---- fragment geometry (transposed reads: lane (g, L) supplies k-row 8g + (L >> 2) and the row 4 below, 8-B piece L & 3)
  const int g = lane >> 4, L = lane & 15;
  const int frow = 8 * g + (L >> 2);
  int aoff[2];
#pragma unroll
  for (int i = 0; i < 2; ++i) aoff[i] = TA::frag_off(frow, wm * 2 + i, L);
  // B fragment of (k32 step ks, tap t, channel tile j): halo row of pixel ks*32 + frow shifted by the tap
  int boff[2][9];                                   // channel tile j = 0; j = 1 is the neighbouring 32-B window: offset ^ 32
#pragma unroll
  for (int ks = 0; ks < 2; ++ks) {
    const int pix = ks * 32 + frow, py = pix / W, px = pix - py * W;
#pragma unroll
    for (int t = 0; t < 9; ++t) {
      const int hr = (py + t / 3) * HW2 + px + t % 3;             // (py + 1 + dy, px + 1 + dx) with dy = t/3 - 1, dx = t%3 - 1
      boff[ks][t] = TA::BYTES + hr * 128 + (((wn * 2) ^ hh(hr)) << 5) + ((L & 3) << 3);
    }
  }
  f32x4 acc[2][9][2];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int t = 0; t < 9; ++t)
#pragma unroll
      for (int j = 0; j < 2; ++j) acc[i][t][j] = f32x4{0.f, 0.f, 0.f, 0.f};
  bf16* const nb = nullptr;

  if (t_begin < t_end) issue(t_begin, 0);
  int slot = 0;
  for (int tile = t_begin; tile < t_end; ++tile, slot ^= 1) {
    asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();                    // tile has landed for every wave; everyone is done reading the slot refilled next
    asm volatile("" ::: "memory");
    if (tile + 1 < t_end) issue(tile + 1, slot ^ 1);
    const char* sS = smem + slot * STAGE;
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) {
      u32x4 fa[2];
#pragma unroll
      for (int i = 0; i < 2; ++i) fa[i] = tr_frag(sS + aoff[i] + ks * 32 * TA::ROWB, TA::ROWB);
#pragma unroll
      for (int t = 0; t < 9; ++t) {
        u32x4 fb[2];
#pragma unroll
        for (int j = 0; j < 2; ++j) fb[j] = tr_frag(sS + (boff[ks][t] ^ (j << 5)), 128);
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
          for (int j = 0; j < 2; ++j) mma16(acc[i][t][j], fa[i], fa[i], fb[j], fb[j], nb);
      }
    }
  }
  const int fr = lane & 15, fg = lane >> 4;
  if (part) {
    // PARTIAL-TILE mode (round 5): the flush of the 64 x 9 x 64 blocks was 35 % of this kernel family (18.6 M fp32 atomics at 192 -> 192 / 32 x 32: 193 us with, 155 us without
    // them; 64 -> 64: 75 / 32 us -- profiles/r05_conv_wgrad_atomics_ablation.txt).  The split's block goes to part[split][N1][N2] in bf16 -- 16 output rows at a time through a
    // per-wave LDS tile [16][9 taps x 32 columns], out as 16-byte pieces (64 contiguous bytes per row and tap) -- and tn_fold_kernel adds the splits in order.
    constexpr int LDP = 9 * 32 + 8;
    __syncthreads();                                    // every wave is done with the dz tiles / halos this overlays
    bf16* const st = (bf16*)smem + wave * 16 * LDP;
    bf16* const P = part + (size_t)bz * p.N1 * p.N2;
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      __builtin_amdgcn_wave_barrier();
#pragma unroll
      for (int t = 0; t < 9; ++t)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
          for (int r = 0; r < 4; ++r) st[(4 * fg + r) * LDP + t * 32 + j * 16 + fr] = (bf16)acc[i][t][j][r];
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
      __builtin_amdgcn_wave_barrier();
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
#pragma unroll
      for (int k = 0; k < 9; ++k) {
        const int q = lane + 64 * k, row = q / 36, rem = q - row * 36, t = rem >> 2, pc = rem & 3;
        const int n1 = o0 + wm * 32 + i * 16 + row, n2 = t * cin + c0 + wn * 32 + pc * 8;
        st_g<MVLT_NT_GEMM>((u32x4*)(P + (size_t)n1 * p.N2 + n2), *(const u32x4*)(st + row * LDP + t * 32 + pc * 8));
      }
    }
    return;
  }
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int t = 0; t < 9; ++t)
#pragma unroll
      for (int j = 0; j < 2; ++j)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int n1 = o0 + wm * 32 + i * 16 + 4 * fg + r;
          const int n2 = t * cin + c0 + wn * 32 + j * 16 + fr;
          atomicAdd(&p.C[(long)n1 * p.ldc + n2], acc[i][t][j][r]);
        }
}

// ------------------------------------------------------------------------------------------------ conv3x3 forward / dgrad, LDS halo
// C[pixel][n] = sum over taps t and channels c of x[pixel + tap t][c] * B[n][t*cin + c]: the MIM decoder's conv3x3 (and its input
// gradient, the same gather with flipped taps) as the NT GEMM with a_map mode 2.  In gemm_nt_dma_kernel every k-step fetches its own
// shifted copy of the 128 input rows through the LDS-DMA path, nine times per 64 channels.  Here the K loop runs channel slice
// outermost: per 64-channel slice the tile's HALO -- (128/W + 2) x (W + 2) input rows, 26 KB at W = 32 -- is loaded once and all
// nine taps read their A fragments from it at shifted row addresses (ds_read_b128, the row's 16-B chunks XOR-swizzled by the halo
// row, conflict-free from any first row); only the weight tiles still stream per k-step.  A traffic per 128 x 192-channel tile: 78 KB instead of 432 KB.  Same tile
// and wave geometry as gemm_nt_dma_kernel (128 x BN, 4 waves, two workgroups per CU), so its epilogues are used unchanged.
template <int W, int BN, int EPI>
__global__ __launch_bounds__(NTHREADS, 2) void conv3_nt_kernel(mvlt_gemm_nt_args p) {
  constexpr int BK = 64, ROWB = 128, CH = 8;
  constexpr int RPL = NTHREADS / CH;
  constexpr int WN = BN / 2, TN_ = WN / 16, TM_ = 4;
  constexpr int B_ITERS = BN * CH / NTHREADS;
  constexpr int R = BM / W, HW2 = W + 2, HR = (R + 2) * HW2;          // image rows per tile; halo rows (one pixel, 64 channels = 128 B)
  constexpr int H_IT = (HR * 8 + NTHREADS - 1) / NTHREADS;
  constexpr int HALO_BYTES = H_IT * NTHREADS * 16;
  constexpr int BSTAGE = BN * ROWB;
  auto swzk = [](int row, int chunk) { return chunk ^ ((row >> 1) & 7); };
  // halo rows are read at arbitrary (tap-shifted) offsets: chunk ^ (((row >> 1) & 3) << 1) keeps every 16-lane group of a
  // ds_read_b128 -- 16 consecutive rows, lanes 4..11 of them one chunk further -- on 16 distinct 16-B bank slots from ANY first row
  // (the (row >> 1) & 7 form used for the 16-aligned tiles is 2-way conflicted from three first rows in four)
  auto swzh = [](int row) { return ((row >> 1) & 3) << 1; };
  extern __shared__ __attribute__((aligned(16))) char smem[];          // [halo slice | B stage 0 | B stage 1]
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm = wave >> 1, wn = wave & 1;
  const int tiles_m = p.M / BM;
  const int tiles_n = (p.N + BN - 1) / BN;
  const int bid = blockIdx.x;
  const int xcd = bid & 7, bgroup = bid >> 3;
  const int tile_m = (bgroup / tiles_n) * 8 + xcd, tile_n = bgroup % tiles_n;
  if (tile_m >= tiles_m) return;
  const int m0 = tile_m * BM, n0 = tile_n * BN;
  const unsigned smem_lds = (unsigned)(uintptr_t)smem;
  const int Himg = p.a_map.h_in, cin = p.a_map.c_seg, tokens_in = p.a_map.tokens_in;
  const int tiles_per_img = Himg * W / BM;
  const int img = tile_m / tiles_per_img, y0 = (tile_m - img * tiles_per_img) * R;
  const char* zsrc = (const char*)g_zero_page + ((tid * 16 + (bid & 15) * 4096) & 65535);
  const unsigned a_rowb = 2u * (unsigned)p.lda;
  const char* img_base = (const char*)p.A + (unsigned long long)(unsigned)(img * tokens_in) * a_rowb;

  // ---- halo loader: LDS row hr = (hy, hx) of the padded window; slot s of row hr holds source chunk swzk(hr, s)
  const char* h_src[H_IT];
#pragma unroll
  for (int j = 0; j < H_IT; ++j) {
    const int q = tid + j * NTHREADS, hr = q >> 3, sl = q & 7;
    const int hy = hr / HW2, hx = hr - hy * HW2;
    const int y = y0 + hy - 1, x = hx - 1;
    const bool ok = hr < HR && (unsigned)y < (unsigned)Himg && (unsigned)x < (unsigned)W;
    h_src[j] = ok ? img_base + (long)(y * W + x) * (long)a_rowb + 2 * ((sl ^ swzh(hr)) << 3) : nullptr;
  }
  auto issue_halo = [&](int kc) {
#pragma unroll
    for (int j = 0; j < H_IT; ++j)
      glds16(h_src[j] ? h_src[j] + kc * 128 : zsrc, __builtin_amdgcn_readfirstlane(smem_lds + (j * NTHREADS + wave * 64) * 16));
  };
  // ---- weight loader (as gemm_nt_dma_kernel): row n of the tile, chunk swizzled by row
  const int row_in = tid / CH;
  const int chunk = swzk(row_in, tid % CH);
  const char* b_ptr[B_ITERS];
  bool b_ok[B_ITERS];
#pragma unroll
  for (int i = 0; i < B_ITERS; ++i) {
    int n = n0 + row_in + RPL * i;
    b_ok[i] = n < p.N;
    b_ptr[i] = (const char*)p.B + (unsigned long long)(unsigned)(b_ok[i] ? n : 0) * (2u * (unsigned)p.ldb) + chunk * 16;
  }
  auto issue_b = [&](int kc, int t, int slot) {
    const int koff = (t * cin + kc * 64) * 2;
#pragma unroll
    for (int i = 0; i < B_ITERS; ++i)
      glds16(b_ok[i] ? b_ptr[i] + koff : zsrc, __builtin_amdgcn_readfirstlane(smem_lds + HALO_BYTES + slot * BSTAGE + (i * NTHREADS + wave * 64) * 16));
  };

  f32x4 acc[TM_][TN_];
#pragma unroll
  for (int i = 0; i < TM_; ++i)
#pragma unroll
    for (int j = 0; j < TN_; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
  const int fr = lane & 15, fg = lane >> 4;
  // halo row of this lane's pixel in each of the wave's four 16-pixel tiles, tap (0, 0)
  int hbase[TM_];
#pragma unroll
  for (int i = 0; i < TM_; ++i) {
    const int pix = wm * 64 + i * 16 + fr, py = pix / W, px = pix - py * W;
    hbase[i] = (py + 1) * HW2 + px + 1;
  }
  const int nkc = cin / 64;
  int bslot = 0;
  for (int kc = 0; kc < nkc; ++kc) {
    // the previous slice's A reads (and the B stage refilled below) are done for every wave
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    issue_halo(kc);
    if (kc == 0) issue_b(0, 0, bslot);                     // later slices: their first weight tile was issued during the previous tap 8
#pragma unroll 1
    for (int t = 0; t < 9; ++t) {
      asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");   // weight tile (kc, t) (and a fresh halo) landed; reads of the other stage done
      __builtin_amdgcn_s_barrier();
      asm volatile("" ::: "memory");
      // all pieces of the next weight tile right behind the barrier: one piece between each pair of MFMA groups instead was 5 % slower
      if (t + 1 < 9) issue_b(kc, t + 1, bslot ^ 1);
      else if (kc + 1 < nkc) issue_b(kc + 1, 0, bslot ^ 1);
      const int tapoff = (t / 3 - 1) * HW2 + (t % 3 - 1);
      const char* b_s = smem + HALO_BYTES + bslot * BSTAGE + (wn * WN) * ROWB;
      bslot ^= 1;
      u32x4 fa[2][TM_], fb[2][TN_];
#pragma unroll
      for (int i = 0; i < TM_; ++i) {
        const int hr = hbase[i] + tapoff;
        const char* rowp = smem + hr * 128;
        const int sw = swzh(hr);
#pragma unroll
        for (int ks = 0; ks < 2; ++ks) fa[ks][i] = *(const u32x4*)(rowp + (((ks * 4 + fg) ^ sw) << 4));
      }
#pragma unroll
      for (int ks = 0; ks < 2; ++ks)
#pragma unroll
        for (int j = 0; j < TN_; ++j) {
          int r = j * 16 + fr;
          fb[ks][j] = *(const u32x4*)(b_s + r * ROWB + swzk(wn * WN + r, ks * 4 + fg) * 16);
        }
#pragma unroll
      for (int ks = 0; ks < 2; ++ks) {
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int i = 0; i < TM_; ++i)
#pragma unroll
          for (int j = 0; j < TN_; ++j) mma16(acc[i][j], fa[ks][i], fa[ks][i], fb[ks][j], fb[ks][j], (bf16*)nullptr);
      }
    }
  }
  __syncthreads();                   // last reads are done before the epilogue reuses the LDS
  if constexpr (BN == 192) nt_epilogue_192<EPI>(p, acc, smem, m0, n0, wave, lane);
  else nt_epilogue_lean<BN, EPI, TM_>(p, acc, smem, m0, n0, wave, lane);
}

}  // namespace

// ------------------------------------------------------------------------------------------------ plan -> launch
int mvlt_launch_nt_conv3(const mvlt_gemm_plan& p, const mvlt_gemm_nt_args& a, hipStream_t s) {
  const char* const who = "mvlt_gemm_nt";
  MVLT_PLAN_LAUNCH_HEAD;
#define NT_CONV3(W_, BN_, EPI_) MVLT_CASE(true, (conv3_nt_kernel<W_, BN_, EPI_>), (MVLT_GEMM_NT_CONV3, W_, BN_, EPI_), a)
#define NT_CONV3_W(W_) NT_CONV3(W_, 192, 1) NT_CONV3(W_, 192, 5) NT_CONV3(W_, 64, 1) NT_CONV3(W_, 64, 2) NT_CONV3(W_, 64, 5) \
                       NT_CONV3(W_, 128, 1) NT_CONV3(W_, 128, 2) NT_CONV3(W_, 128, 5)
  switch (key) {
    NT_CONV3_W(32) NT_CONV3_W(16) NT_CONV3_W(64)
  }
  return no_instantiation(who, p);
}

int mvlt_launch_tn_conv3(const mvlt_gemm_plan& p, const mvlt_gemm_tn_args& k, bf16* part, hipStream_t s) {
  const char* const who = "mvlt_gemm_tn";
  MVLT_PLAN_LAUNCH_HEAD;
#define TN_CONV3(W_) MVLT_CASE(true, (conv3_wgrad_kernel<W_>), (MVLT_GEMM_TN_CONV3, W_), k, p.per_split, p.t1, p.t2, p.splits, part)
  switch (key) {
    TN_CONV3(64) TN_CONV3(32) TN_CONV3(16) TN_CONV3(8)
  }
  return no_instantiation(who, p);
}

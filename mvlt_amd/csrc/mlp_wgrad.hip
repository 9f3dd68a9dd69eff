// Fused MLP of stages 1-2, weight gradients: mlp_wgrad_kernel (DropPath factor per row), mlp_wgrad2_kernel (factor per 64-token tile, activation by table; optionally
// bf16 partial tiles + two ordered folds instead of fp32 atomics) and their launch.  Overview: mlp.hip; dispatch: mlp_plan.h.
#include "mlp_common.h"

namespace {

// Activation by table (mlp_wgrad2_kernel): the pre-activation is rounded to bf16 -- what the stage 3-4 path stores and what torch autocast hands nn.GELU -- and
// { Phi - 1/2, GELU' - 1/2 } of its magnitude comes out of a 13 KB LDS copy of g_gelu_lut (tools/gen_gelu_lut.py); the sign is applied by one FMA each: 9.5 VALU
// instructions + one ds_read_b64 per hidden activation instead of the sigmoid form's 17.  Measured (same box, tools/ubench_mlp2.py / ab_bench_libs.sh): weight gradients
// 470 -> 363 us (C = 64) and 381 -> 358 us (C = 128), step -0.24 ms.  The forward and input-gradient kernels keep the polynomial (mlp_pipe.hip has their figures).
#include "gelu_lut.inc"
using mvlt_mlp::GELU_LUT_BYTES;
static_assert(GELU_LUT_BYTES == MVLT_GELU_LUT_PAD * 8 && GELU_LUT_BYTES % 1024 == 0, "mlp_common.h sizes the LDS for this table: whole 1 KB LDS-DMA instructions");
// the table into LDS by LDS-DMA, 1 KB per wave instruction, dealt round-robin to the NWV waves (lands with the kernel's first vmcnt(0) + barrier)
template <int NWV> __device__ __forceinline__ void gelu_lut_dma(unsigned lds_base, int wave, int lane) {
  for (int k = wave; k < GELU_LUT_BYTES / 1024; k += NWV)
    glds16((const char*)&g_gelu_lut[0][0] + k * 1024 + lane * 16, __builtin_amdgcn_readfirstlane(lds_base + k * 1024));
}
// index of a bf16 magnitude (15 bits) as a byte offset from lut0 = table base - 8 * MVLT_GELU_LUT_BASE
__device__ __forceinline__ unsigned gelu_lut_off(unsigned u) {
  return min(max(u, (unsigned)MVLT_GELU_LUT_BASE), (unsigned)MVLT_GELU_LUT_TOP) << 3;
}
__device__ __forceinline__ float gelu_lut_sign(float h) { return __builtin_bit_cast(float, (__builtin_bit_cast(unsigned, h) & 0x80000000u) | 0x3f800000u); }
// Phi(h) and GELU'(h) of two pre-activations; lut0 = LDS table base - 8 * MVLT_GELU_LUT_BASE
__device__ __forceinline__ void gelu_lut_both2(const char* lut0, float h0, float h1, float& ph0, float& d0, float& ph1, float& d1) {
  const unsigned pk = __builtin_bit_cast(unsigned, __builtin_convertvector(f32x2{h0, h1}, bf16x2));
  const f32x2 t0 = *(const f32x2*)(lut0 + gelu_lut_off(pk & 0x7fffu)), t1 = *(const f32x2*)(lut0 + gelu_lut_off((pk >> 16) & 0x7fffu));
  const float s0 = gelu_lut_sign(h0), s1 = gelu_lut_sign(h1);
  ph0 = __builtin_fmaf(s0, t0[0], 0.5f); d0 = __builtin_fmaf(s0, t0[1], 0.5f);
  ph1 = __builtin_fmaf(s1, t1[0], 0.5f); d1 = __builtin_fmaf(s1, t1[1], 0.5f);
}

// ------------------------------------------------------------------------------------------------ weight gradients
// dW1[j][c] += sum_m dh[m][j] x[m][c]      db1[j] += sum_m dh[m][j]
// dW2[c][j] += sum_m dy[m][c] g[m][j]      db2[c] += sum_m dy[m][c]          (dy scaled by the per-sample DropPath factor)
// A workgroup owns 128 hidden units and a range of tokens; W1 / W2^T rows of its hidden range stay in LDS.  Per 64-token
// tile it recomputes h and dg for its hidden units (MFMA, rows = tokens), turns them into g and dh in registers and
// feeds those straight back as MFMA operands of the two weight-gradient products (k = tokens): the C layout (4
// consecutive tokens per lane) IS the operand layout once two 16-token tiles are paired.  The other operands, x^T / dy^T
// fragments, are transposed reads (ds_read_b64_tr_b16) of the same natural-layout [token][C] tiles the producers read
// row-wise; those tiles arrive by LDS-DMA in a 2-deep ring (the kernel runs one or two waves per SIMD: without the
// prefetch every tile paid a full HBM/L2 round trip).  Nothing of size (tokens x hidden) is ever written.
//
// Tile layout: row = token, 16-B chunks XOR-swizzled by hs(token) << 1 on the DMA source side; hs is chosen so that
// both access patterns are bank-conflict free: the b128 row reads (16 tokens x 4 chunks per instruction) and the
// transposed reads (8 consecutive tokens x one 32-B window per 32-lane group).
template <int C> __device__ __forceinline__ int wg_hs(int row) { return C == 64 ? ((row >> 1) & 3) : (row & 7); }

__device__ __forceinline__ float sload_f32(const float* ptr) {      // scalar load: must not touch vmcnt (the DMA ring counts it)
  float v;
  asm volatile("s_load_dword %0, %1, 0x0\n\ts_waitcnt lgkmcnt(0)" : "=s"(v) : "s"(ptr) : "memory");
  return v;
}

template <int C>
__global__ __launch_bounds__(NT, C == 64 ? 2 : 1) void mlp_wgrad_kernel(mvlt_mlp_args p, int m_per_split, int splits, int ny) {
  constexpr int KS_C = C / 32, CT16 = C / 16;
  constexpr int ROWB = 2 * C;                  // bytes per token row
  constexpr int CH = C / 8;                    // 16-B slots per row
  constexpr int RPP = NT / CH;                 // rows per 256-thread pass
  constexpr int IT = 64 / RPP;                 // passes per tile
  constexpr int TILE = 64 * ROWB;
  constexpr int STAGE = 2 * TILE;              // x tile | dy tile
  constexpr int LPT = 2 * IT;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  bf16* sW1 = (bf16*)smem;                     // [128][C]
  bf16* sW2T = sW1 + 128 * C;                  // [128][C]
  char* sT = smem + 2 * 128 * C * 2;           // [2][x tile | dy tile]
  static_assert(2 * 128 * C * 2 + 2 * STAGE == mvlt_mlp::wgrad_lds(C), "the plan sizes this launch with mlp_common.h's formula");
  const unsigned sT_lds = (unsigned)(uintptr_t)sT;

  // one token split (all its ny hidden blocks) per XCD: x / dy rows come through that L2 once
  const int xcd = blockIdx.x & 7, kq = blockIdx.x >> 3;
  const int zq = kq / ny, by = kq - zq * ny;
  const int bz = zq * 8 + xcd;
  if (bz >= splits) return;

  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int fr = lane & 15, fg = lane >> 4;
  const int j0 = by * 128;
  const int m_begin = bz * m_per_split, m_end = min(p.M, m_begin + m_per_split);

  // ---- DMA geometry
  const int l_row0 = tid / CH;
  const int l_chunk = (tid % CH) ^ (wg_hs<C>(l_row0) << 1);
  const char* xsrc = (const char*)p.x + l_chunk * 16;
  const char* ysrc = (const char*)p.dy + l_chunk * 16;
  const char* zsrc = (const char*)g_zero_page + ((tid * 16 + (blockIdx.x & 15) * 4096) & 65535);
  auto issue = [&](int mt, int slot) {
#pragma unroll
    for (int j = 0; j < IT; ++j) {
      const int m = mt + j * RPP + l_row0;
      const bool ok = m < m_end;
      const unsigned long long off = (unsigned long long)(unsigned)m * ROWB;
      const unsigned dst = __builtin_amdgcn_readfirstlane(sT_lds + slot * STAGE + (j * NT + wave * 64) * 16);
      glds16(ok ? xsrc + off : zsrc, dst);
      glds16(ok ? ysrc + off : zsrc, dst + TILE);
    }
  };
  issue(m_begin, 0);

  for (int u = tid; u < 128 * (C / 8); u += NT) {
    int r = u / (C / 8), ch = u % (C / 8);
    *(u32x4*)(sW1 + toff<C>(r, ch * 8)) = *(const u32x4*)((const bf16*)p.w1 + (long)(j0 + r) * C + ch * 8);
    *(u32x4*)(sW2T + toff<C>(r, ch * 8)) = *(const u32x4*)((const bf16*)p.wc + (long)(j0 + r) * C + ch * 8);
  }
  float b1v[2];
#pragma unroll
  for (int jt = 0; jt < 2; ++jt) b1v[jt] = p.b1[j0 + wave * 32 + jt * 16 + fr];
  asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
  __syncthreads();                             // weights visible (and tile 0 has landed)

  // ---- fragment geometry
  const int hs_row = wg_hs<C>(fr);                                   // producers: token row 16 mt + fr
  int xoff[KS_C];
#pragma unroll
  for (int ks = 0; ks < KS_C; ++ks) xoff[ks] = fr * ROWB + (((ks * 4 + fg) ^ (hs_row << 1)) << 4);
  const int L = lane & 15;
  const int trow = 4 * fg + (L >> 2);                                // transposed reads: token row 32 pair + trow (+16)
  const int hs_t = wg_hs<C>(trow);
  int toffs[CT16];
#pragma unroll
  for (int ct = 0; ct < CT16; ++ct) toffs[ct] = trow * ROWB + ((ct ^ hs_t) << 5) + ((L & 3) << 3);

  f32x4 dw1[2][CT16], dw2[CT16][2];
#pragma unroll
  for (int a = 0; a < 2; ++a)
#pragma unroll
    for (int b = 0; b < CT16; ++b) { dw1[a][b] = f32x4{0.f, 0.f, 0.f, 0.f}; dw2[b][a] = f32x4{0.f, 0.f, 0.f, 0.f}; }
  float db1acc[2] = {0.f, 0.f};
  float db2acc[CT16 / 4];
#pragma unroll
  for (int b = 0; b < CT16 / 4; ++b) db2acc[b] = 0.f;
  const bool do_db2 = by == 0;                 // column sums of dy: the four waves take every fourth 16-channel tile each
  const bool scaled = p.row_scale != nullptr;

  int slot = 0;
  for (int mt0 = m_begin; mt0 < m_end; mt0 += 64, slot ^= 1) {
    if (mt0 != m_begin) {
      asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
      __builtin_amdgcn_s_barrier();            // tile mt0 landed for every wave; the other slot is free again
      asm volatile("" ::: "memory");
    }
    if (mt0 + 64 < m_end) issue(mt0 + 64, slot ^ 1);
    const char* tX = sT + slot * STAGE;
    const char* tY = tX + TILE;

    // per-sample DropPath factor of this lane's 16 token rows (16 mt + 4 fg + r).  From 63 rows per sample on a 64-row tile spans at most two samples:
    // two scalar loads and a compare per row.  Shorter samples (stage 2 of a 64 x 32 px input with T = 20 has 52 rows per sample: a tile can hold the tail of
    // one, all of the next and the head of a third) look the factor up per row; the index is clamped to the last sample for the rows past M, which hold zeros.
    float sc[4][4];
    if (scaled && p.rows_per_scale < 63) {
      const int last = (p.M - 1) / p.rows_per_scale;
#pragma unroll
      for (int mt = 0; mt < 4; ++mt)
#pragma unroll
        for (int r = 0; r < 4; ++r) sc[mt][r] = p.row_scale[min((mt0 + mt * 16 + 4 * fg + r) / p.rows_per_scale, last)];
    } else if (scaled) {
      const int b0 = __builtin_amdgcn_readfirstlane(mt0 / p.rows_per_scale);
      const int bound = (b0 + 1) * p.rows_per_scale;
      const int b1i = __builtin_amdgcn_readfirstlane(min(b0 + 1, (p.M - 1) / p.rows_per_scale));
      const float sA = sload_f32(p.row_scale + b0), sB = sload_f32(p.row_scale + b1i);
#pragma unroll
      for (int mt = 0; mt < 4; ++mt)
#pragma unroll
        for (int r = 0; r < 4; ++r) sc[mt][r] = (mt0 + mt * 16 + 4 * fg + r < bound) ? sA : sB;
    }

    // ---- producers: h, dg for this wave's 32 hidden units x 64 tokens; rows = tokens (4 fg + r), cols = hidden (fr)
    bf16x8 gfrag[2][2], dhfrag[2][2];          // [hidden tile][token-tile pair]: k-slot (fg, jj) <-> token 32 pair + 16 (jj>>2) + 4 fg + (jj&3)
    bf16x8 w1f[2][KS_C], w2f[2][KS_C];
#pragma unroll
    for (int jt = 0; jt < 2; ++jt)
#pragma unroll
      for (int ks = 0; ks < KS_C; ++ks) {
        w1f[jt][ks] = ldfrag(sW1 + toff<C>(wave * 32 + jt * 16 + fr, ks * 32 + fg * 8));
        w2f[jt][ks] = ldfrag(sW2T + toff<C>(wave * 32 + jt * 16 + fr, ks * 32 + fg * 8));
      }
#pragma unroll
    for (int mt = 0; mt < 4; ++mt) {
      bf16x8 xf[KS_C], yf[KS_C];
#pragma unroll
      for (int ks = 0; ks < KS_C; ++ks) {
        xf[ks] = *(const bf16x8*)(tX + mt * 16 * ROWB + xoff[ks]);
        yf[ks] = *(const bf16x8*)(tY + mt * 16 * ROWB + xoff[ks]);
      }
#pragma unroll
      for (int jt = 0; jt < 2; ++jt) {
        f32x4 h = {0.f, 0.f, 0.f, 0.f}, dg = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int ks = 0; ks < KS_C; ++ks) {
          h = __builtin_amdgcn_mfma_f32_16x16x32_bf16(xf[ks], w1f[jt][ks], h, 0, 0, 0);
          dg = __builtin_amdgcn_mfma_f32_16x16x32_bf16(yf[ks], w2f[jt][ks], dg, 0, 0, 0);
        }
#pragma unroll
        for (int r = 0; r < 4; r += 2) {
          const f32x2 hv = f32x2{h[r], h[r + 1]} + b1v[jt];
          f32x2 gv, dgv;
          gelu_fast_both2(hv, gv, dgv);
          f32x2 dhv = f32x2{dg[r], dg[r + 1]} * dgv;
          if (scaled) {                        // dy's factor moves onto the two products it enters linearly
            const f32x2 s2 = {sc[mt][r], sc[mt][r + 1]};
            dhv *= s2; gv *= s2;
          }
          db1acc[jt] += dhv[0] + dhv[1];
          gfrag[jt][mt >> 1][(mt & 1) * 4 + r] = (bf16)gv[0];
          gfrag[jt][mt >> 1][(mt & 1) * 4 + r + 1] = (bf16)gv[1];
          dhfrag[jt][mt >> 1][(mt & 1) * 4 + r] = (bf16)dhv[0];
          dhfrag[jt][mt >> 1][(mt & 1) * 4 + r + 1] = (bf16)dhv[1];
        }
      }
    }
    // ---- weight-gradient products, k = tokens (two k32 steps per 64-token tile)
#pragma unroll
    for (int pair = 0; pair < 2; ++pair) {
#pragma unroll
      for (int ct = 0; ct < CT16; ++ct) {
        typedef __attribute__((address_space(3))) s16x4* lptr;
        const char* ax = tX + pair * 32 * ROWB + toffs[ct];
        const char* ay = tY + pair * 32 * ROWB + toffs[ct];
        s16x4 xa = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lptr)ax), xb = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lptr)(ax + 16 * ROWB));
        s16x4 ya = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lptr)ay), yb = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lptr)(ay + 16 * ROWB));
        const unsigned long long xl = __builtin_bit_cast(unsigned long long, xa), xh = __builtin_bit_cast(unsigned long long, xb);
        const unsigned long long yl = __builtin_bit_cast(unsigned long long, ya), yh = __builtin_bit_cast(unsigned long long, yb);
        const bf16x8 xt = __builtin_bit_cast(bf16x8, u32x4{(unsigned)xl, (unsigned)(xl >> 32), (unsigned)xh, (unsigned)(xh >> 32)});
        const bf16x8 yt = __builtin_bit_cast(bf16x8, u32x4{(unsigned)yl, (unsigned)(yl >> 32), (unsigned)yh, (unsigned)(yh >> 32)});
        if (do_db2 && (ct & 3) == wave) {
#pragma unroll
          for (int e = 0; e < 8; ++e) {
            const float sv = scaled ? sc[2 * pair + (e >> 2)][e & 3] : 1.0f;
            db2acc[ct >> 2] += (float)yt[e] * sv;
          }
        }
#pragma unroll
        for (int jt = 0; jt < 2; ++jt) {
          dw1[jt][ct] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(dhfrag[jt][pair], xt, dw1[jt][ct], 0, 0, 0);   // rows j, cols c
          dw2[ct][jt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(yt, gfrag[jt][pair], dw2[ct][jt], 0, 0, 0);    // rows c, cols j
        }
      }
    }
  }
  // ---- flush
#pragma unroll
  for (int jt = 0; jt < 2; ++jt) {
    const int jb = j0 + wave * 32 + jt * 16;
#pragma unroll
    for (int ct = 0; ct < CT16; ++ct)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        atomicAdd(&p.dw1[(long)(jb + 4 * fg + r) * C + ct * 16 + fr], dw1[jt][ct][r]);
        atomicAdd(&p.dw2[(long)(ct * 16 + 4 * fg + r) * p.hid + jb + fr], dw2[ct][jt][r]);
      }
    float v = db1acc[jt];
    v += __shfl_xor(v, 16);
    v += __shfl_xor(v, 32);
    if (fg == 0) atomicAdd(&p.db1[jb + fr], v);
  }
  if (do_db2) {
#pragma unroll
    for (int q = 0; q < CT16 / 4; ++q) {
      float v = db2acc[q];
      v += __shfl_xor(v, 16);
      v += __shfl_xor(v, 32);
      if (fg == 0) atomicAdd(&p.db2[(q * 4 + wave) * 16 + fr], v);
    }
  }
}

// ---- round 3: the same computation with (a) the activation's VALU work of token sub-tile mt issued in the shadow of sub-tile mt + 1's
// producer MFMAs and of the weight-gradient MFMAs (slots pinned by sched_barrier(0), as in mlp_pipe_kernel), (b) the per-sample
// DropPath factor taken per 64-token TILE (mlp_plan.h takes this path when a sample is whole tiles long: a tile then never straddles two
// samples): one scalar per tile instead of sixteen compare / select pairs, and a tile whose factor is 0 -- the sample's branch was
// dropped -- is skipped altogether, (c) fc1's bias as the producers' accumulator initialiser and db1 = dh^T 1 as one more MFMA column
// block instead of VALU adds, (d) NW = 8 waves of ONE 16-unit hidden tile each at C = 128, where the four-wave form needs 446 registers
// per lane (one wave per SIMD: a VALU-bound loop then issues one instruction per ~7 cycles instead of one per ~3).
template <int C, int NW>
__global__ __launch_bounds__(NW * 64, NW == 8 ? 2 : 2) void mlp_wgrad2_kernel(mvlt_mlp_args p, int m_per_split, int splits, int ny, void* part1_, void* part2_) {
  // (void*: a __bf16* parameter makes rocprofv3 print the kernel's MANGLED name -- its demangler does not know DF16b -- and every name-keyed tool of tools/ loses the kernel)
  bf16* const part1 = (bf16*)part1_;
  bf16* const part2 = (bf16*)part2_;
  constexpr int NTH = NW * 64;
  constexpr int JT = 8 / NW;                   // 16-unit hidden tiles per wave: 2 (4 waves) / 1 (8 waves)
  constexpr int KS_C = C / 32, CT16 = C / 16;
  constexpr int ROWB = 2 * C;                  // bytes per token row
  constexpr int CH = C / 8;                    // 16-B slots per row
  constexpr int RPP = NTH / CH;                // rows per pass of the whole workgroup
  constexpr int IT = 64 / RPP;                 // passes per tile
  constexpr int TILE = 64 * ROWB;
  constexpr int STAGE = 2 * TILE;              // x tile | dy tile
  extern __shared__ __attribute__((aligned(16))) char smem[];
  bf16* sW1 = (bf16*)smem;                     // [128][C]
  bf16* sW2T = sW1 + 128 * C;                  // [128][C]
  char* sT = smem + 2 * 128 * C * 2;           // [2][x tile | dy tile]
  constexpr int TILE_ = 64 * 2 * C;
  float* sLut = (float*)(sT + 2 * 2 * TILE_);  // activation table
  static_assert(2 * 128 * C * 2 + 2 * 2 * TILE_ + GELU_LUT_BYTES == mvlt_mlp::wgrad2_lds(C, NW) && NW == mvlt_mlp::wgrad2_waves(C),
                "the plan sizes this launch with mlp_common.h's formula");
  const char* const lut0 = (const char*)sLut - 8 * MVLT_GELU_LUT_BASE;
  const unsigned sT_lds = (unsigned)(uintptr_t)sT;

  // one token split (all its ny hidden blocks) per XCD: x / dy rows come through that L2 once
  const int xcd = blockIdx.x & 7, kq = blockIdx.x >> 3;
  const int zq = kq / ny, by = kq - zq * ny;
  const int bz = zq * 8 + xcd;
  if (bz >= splits) return;

  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int fr = lane & 15, fg = lane >> 4;
  const int j0 = by * 128, jw = wave * 16 * JT;                   // this wave's hidden units: j0 + jw + 16 jt + (column)
  const int m_begin = bz * m_per_split, m_end = min(p.M, m_begin + m_per_split);

  // ---- DMA geometry (same image as mlp_wgrad_kernel)
  const int l_row0 = tid / CH;
  const int l_chunk = (tid % CH) ^ (wg_hs<C>(l_row0) << 1);
  const char* xsrc = (const char*)p.x + l_chunk * 16;
  const char* ysrc = (const char*)p.dy + l_chunk * 16;
  const char* zsrc = (const char*)g_zero_page + ((tid * 16 + (blockIdx.x & 15) * 4096) & 65535);
  auto issue = [&](int mt, int slot) {
#pragma unroll
    for (int j = 0; j < IT; ++j) {
      const int m = mt + j * RPP + l_row0;
      const bool ok = m < m_end;
      const unsigned long long off = (unsigned long long)(unsigned)m * ROWB;
      const unsigned dst = __builtin_amdgcn_readfirstlane(sT_lds + slot * STAGE + (j * NTH + wave * 64) * 16);
      glds16(ok ? xsrc + off : zsrc, dst);
      glds16(ok ? ysrc + off : zsrc, dst + TILE);
    }
  };
  issue(m_begin, 0);

  for (int u = tid; u < 128 * (C / 8); u += NTH) {
    int r = u / (C / 8), ch = u % (C / 8);
    *(u32x4*)(sW1 + toff<C>(r, ch * 8)) = *(const u32x4*)((const bf16*)p.w1 + (long)(j0 + r) * C + ch * 8);
    *(u32x4*)(sW2T + toff<C>(r, ch * 8)) = *(const u32x4*)((const bf16*)p.wc + (long)(j0 + r) * C + ch * 8);
  }
  gelu_lut_dma<NW>((unsigned)(uintptr_t)sLut, wave, lane);
  float b1v[JT];
#pragma unroll
  for (int jt = 0; jt < JT; ++jt) b1v[jt] = p.b1[j0 + jw + jt * 16 + fr];
  asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
  __syncthreads();                             // weights visible (and tile 0 has landed)

  // ---- fragment geometry
  const int hs_row = wg_hs<C>(fr);                                   // producers: token row 16 mt + fr
  int xoff[KS_C];
#pragma unroll
  for (int ks = 0; ks < KS_C; ++ks) xoff[ks] = fr * ROWB + (((ks * 4 + fg) ^ (hs_row << 1)) << 4);
  const int L = lane & 15;
  const int trow = 4 * fg + (L >> 2);                                // transposed reads: token row 32 pair + trow (+16)
  const int hs_t = wg_hs<C>(trow);
  int toffs[CT16];
#pragma unroll
  for (int ct = 0; ct < CT16; ++ct) toffs[ct] = trow * ROWB + ((ct ^ hs_t) << 5) + ((L & 3) << 3);

  // the hidden-unit operands of the producers stay in registers: 2 JT KS_C fragments (32 registers at either geometry)
  bf16x8 w1f[JT][KS_C], w2f[JT][KS_C];
#pragma unroll
  for (int jt = 0; jt < JT; ++jt)
#pragma unroll
    for (int ks = 0; ks < KS_C; ++ks) {
      w1f[jt][ks] = ldfrag(sW1 + toff<C>(jw + jt * 16 + fr, ks * 32 + fg * 8));
      w2f[jt][ks] = ldfrag(sW2T + toff<C>(jw + jt * 16 + fr, ks * 32 + fg * 8));
    }

  f32x4 dw1[JT][CT16], dw2[CT16][JT], db1m[JT];
#pragma unroll
  for (int a = 0; a < JT; ++a) {
    db1m[a] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int b = 0; b < CT16; ++b) { dw1[a][b] = f32x4{0.f, 0.f, 0.f, 0.f}; dw2[b][a] = f32x4{0.f, 0.f, 0.f, 0.f}; }
  }
  // db2[c] = sum_m s_m dy[m][c]: wave w owns channel tile w (CT16 == NW at both geometries) and adds one MFMA against a ones fragment per
  // token-tile pair -- every column of that product holds the row sums.  Every workgroup computes it (two MFMAs per tile, no branch in
  // the loop); the by == 0 ones flush it.
  // The per-sample factor s never touches the per-element path: the accumulators hold UNSCALED sums under the invariant
  // true sum = run_sc x accumulator.  Tiles of dropped samples (s = 0) are skipped; when a tile's factor differs from run_sc (DropPath
  // hands out one non-zero value per block, so in practice never) the accumulators are rescaled by run_sc / s first.  The flush multiplies
  // by run_sc.
  static_assert(CT16 == NW, "one channel tile of dy per wave");
  f32x4 db2m = {0.f, 0.f, 0.f, 0.f};
  float run_sc = 0.0f;                         // 0: nothing accumulated yet
  const int toff_own = trow * ROWB + ((wave ^ hs_t) << 5) + ((L & 3) << 3);
  const bool do_db2 = by == 0;
  const bool scaled = p.row_scale != nullptr;
  const bf16x8 ones = {(bf16)1.f, (bf16)1.f, (bf16)1.f, (bf16)1.f, (bf16)1.f, (bf16)1.f, (bf16)1.f, (bf16)1.f};

  int slot = 0;
  for (int mt0 = m_begin; mt0 < m_end; mt0 += 64, slot ^= 1) {
    if (mt0 != m_begin) {
      asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
      __builtin_amdgcn_s_barrier();            // tile mt0 landed for every wave; the other slot is free again
      asm volatile("" ::: "memory");
    }
    if (mt0 + 64 < m_end) issue(mt0 + 64, slot ^ 1);
    // DropPath factor of this tile's sample (wave-uniform); a dropped sample contributes nothing to any of the four gradients
    float sc = 1.0f;
    if (scaled) {
      sc = sload_f32(p.row_scale + __builtin_amdgcn_readfirstlane(mt0 / p.rows_per_scale));
      if (sc == 0.0f) continue;
    }
    if (sc != run_sc) {
      if (run_sc != 0.0f) {
        const float f = run_sc / sc;
#pragma unroll
        for (int a = 0; a < JT; ++a) {
          db1m[a] *= f;
#pragma unroll
          for (int b = 0; b < CT16; ++b) { dw1[a][b] *= f; dw2[b][a] *= f; }
        }
        db2m *= f;
      }
      run_sc = sc;
    }
    const char* tX = sT + slot * STAGE;
    const char* tY = tX + TILE;

    f32x4 hd[2][JT][2];                        // [sub-tile parity][hidden tile][h | dg]
    u32x4 gfrag[JT][2], dhfrag[JT][2];         // [hidden tile][token-tile pair]: k-slot (fg, jj) <-> token 32 pair + 16 (jj>>2) + 4 fg + (jj&3)
    auto produce = [&](auto mtc) {
      constexpr int mt = decltype(mtc)::value;
      bf16x8 xf[KS_C], yf[KS_C];
#pragma unroll
      for (int ks = 0; ks < KS_C; ++ks) {
        xf[ks] = *(const bf16x8*)(tX + mt * 16 * ROWB + xoff[ks]);
        yf[ks] = *(const bf16x8*)(tY + mt * 16 * ROWB + xoff[ks]);
      }
#pragma unroll
      for (int jt = 0; jt < JT; ++jt) {
        f32x4 h = {b1v[jt], b1v[jt], b1v[jt], b1v[jt]}, dg = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int ks = 0; ks < KS_C; ++ks) {
          h = __builtin_amdgcn_mfma_f32_16x16x32_bf16(xf[ks], w1f[jt][ks], h, 0, 0, 0);
          dg = __builtin_amdgcn_mfma_f32_16x16x32_bf16(yf[ks], w2f[jt][ks], dg, 0, 0, 0);
        }
        hd[mt & 1][jt][0] = h;
        hd[mt & 1][jt][1] = dg;
      }
    };
    auto activate = [&](auto mtc) {
      constexpr int mt = decltype(mtc)::value;
#pragma unroll
      for (int jt = 0; jt < JT; ++jt)
#pragma unroll
        for (int r = 0; r < 4; r += 2) {
          const float h0 = hd[mt & 1][jt][0][r], h1 = hd[mt & 1][jt][0][r + 1];
          float ph0, ph1, d0, d1;
          gelu_lut_both2(lut0, h0, h1, ph0, d0, ph1, d1);
          const float g0 = h0 * ph0, g1 = h1 * ph1;
          const float q0 = hd[mt & 1][jt][1][r], q1 = hd[mt & 1][jt][1][r + 1];
          gfrag[jt][mt >> 1][(mt & 1) * 2 + (r >> 1)] = __builtin_bit_cast(unsigned, __builtin_convertvector(f32x2{g0, g1}, bf16x2));
          dhfrag[jt][mt >> 1][(mt & 1) * 2 + (r >> 1)] = __builtin_bit_cast(unsigned, __builtin_convertvector(f32x2{q0 * d0, q1 * d1}, bf16x2));
        }
    };
    auto consume = [&](auto pairc, auto ct0c, auto ct1c) {       // weight-gradient products of token-tile pair `pair`, channel tiles [ct0, ct1)
      constexpr int pair = decltype(pairc)::value, ct0 = decltype(ct0c)::value, ct1 = decltype(ct1c)::value;
#pragma unroll
      for (int ct = ct0; ct < ct1; ++ct) {
        typedef __attribute__((address_space(3))) s16x4* lptr;
        const char* ax = tX + pair * 32 * ROWB + toffs[ct];
        const char* ay = tY + pair * 32 * ROWB + toffs[ct];
        s16x4 xa = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lptr)ax), xb = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lptr)(ax + 16 * ROWB));
        s16x4 ya = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lptr)ay), yb = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lptr)(ay + 16 * ROWB));
        const unsigned long long xl = __builtin_bit_cast(unsigned long long, xa), xh = __builtin_bit_cast(unsigned long long, xb);
        const unsigned long long yl = __builtin_bit_cast(unsigned long long, ya), yh = __builtin_bit_cast(unsigned long long, yb);
        const bf16x8 xt = __builtin_bit_cast(bf16x8, u32x4{(unsigned)xl, (unsigned)(xl >> 32), (unsigned)xh, (unsigned)(xh >> 32)});
        const bf16x8 yt = __builtin_bit_cast(bf16x8, u32x4{(unsigned)yl, (unsigned)(yl >> 32), (unsigned)yh, (unsigned)(yh >> 32)});
#pragma unroll
        for (int jt = 0; jt < JT; ++jt) {
          dw1[jt][ct] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, dhfrag[jt][pair]), xt, dw1[jt][ct], 0, 0, 0);   // rows j, cols c
          dw2[ct][jt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(yt, __builtin_bit_cast(bf16x8, gfrag[jt][pair]), dw2[ct][jt], 0, 0, 0);    // rows c, cols j
        }
      }
      if (ct0 == 0) {
#pragma unroll
        for (int jt = 0; jt < JT; ++jt)        // db1[j] += sum over the pair's 32 tokens of dh: one more column block, against ones
          db1m[jt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, dhfrag[jt][pair]), ones, db1m[jt], 0, 0, 0);
        typedef __attribute__((address_space(3))) s16x4* lptr;
        const char* ay = tY + pair * 32 * ROWB + toff_own;
        s16x4 ya = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lptr)ay), yb = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lptr)(ay + 16 * ROWB));
        const unsigned long long yl = __builtin_bit_cast(unsigned long long, ya), yh = __builtin_bit_cast(unsigned long long, yb);
        const bf16x8 yo = __builtin_bit_cast(bf16x8, u32x4{(unsigned)yl, (unsigned)(yl >> 32), (unsigned)yh, (unsigned)(yh >> 32)});
        db2m = __builtin_amdgcn_mfma_f32_16x16x32_bf16(yo, ones, db2m, 0, 0, 0);
      }
    };
    using I0 = std::integral_constant<int, 0>;
    using I1 = std::integral_constant<int, 1>;
    using I2 = std::integral_constant<int, 2>;
    using I3 = std::integral_constant<int, 3>;
    using IH = std::integral_constant<int, CT16 / 2>;
    using IF = std::integral_constant<int, CT16>;
    produce(I0{});
    __builtin_amdgcn_sched_barrier(0);
    produce(I1{}); activate(I0{});
    __builtin_amdgcn_sched_barrier(0);
    produce(I2{}); activate(I1{});
    __builtin_amdgcn_sched_barrier(0);
    produce(I3{}); consume(I0{}, I0{}, IH{}); activate(I2{});
    __builtin_amdgcn_sched_barrier(0);
    consume(I0{}, IH{}, IF{}); activate(I3{});
    __builtin_amdgcn_sched_barrier(0);
    consume(I1{}, I0{}, IF{});
  }
  // ---- flush (true sums = run_sc x accumulators)
  if (part1) {
    // round 6: no atomics for the two weight gradients -- this token split's sums leave as bf16 PARTIAL tiles, part1[bz][hid][C] and part2[bz][C][hid], and the ordered fold of
    // the TN GEMMs (tn_fold_multi_kernel) adds the splits into dw1 / dw2: 8.4 M fp32 atomics per launch less, and bit-identical fc gradients from run to run.  Through a
    // per-wave LDS tile so that the partials leave as 16-byte pieces of contiguous rows (the operand tiles are dead: every wave is past the token loop).
    constexpr int LD1 = C + 8;                 // dW1 rows: [16 hidden units][C]
    constexpr int LD2 = 16 * JT + 8;           // dW2 rows: [16 channels][this wave's 16 JT hidden units]
    constexpr int PERW = 16 * (LD1 > LD2 ? LD1 : LD2);
    static_assert(NW * PERW * sizeof(bf16) == mvlt_mlp::wgrad2_flush_bytes(C, NW), "mlp_common.h's wgrad2_lds covers this staging");
    asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
    __syncthreads();
    bf16* const st = (bf16*)smem + wave * PERW;
    bf16* const P1 = part1 + (size_t)bz * p.hid * C;
    bf16* const P2 = part2 + (size_t)bz * p.hid * C;
#pragma unroll
    for (int jt = 0; jt < JT; ++jt) {
      const int jb = j0 + jw + jt * 16;
      __builtin_amdgcn_wave_barrier();
#pragma unroll
      for (int ct = 0; ct < CT16; ++ct)
#pragma unroll
        for (int r = 0; r < 4; ++r) st[(4 * fg + r) * LD1 + ct * 16 + fr] = (bf16)(dw1[jt][ct][r] * run_sc);
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
      __builtin_amdgcn_wave_barrier();
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
#pragma unroll
      for (int q = lane; q < 16 * (C / 8); q += 64) {
        const int row = q / (C / 8), ch = q - row * (C / 8);
        *(u32x4*)(P1 + (size_t)(jb + row) * C + ch * 8) = *(const u32x4*)(st + row * LD1 + ch * 8);
      }
    }
#pragma unroll
    for (int ct = 0; ct < CT16; ++ct) {
      __builtin_amdgcn_wave_barrier();
#pragma unroll
      for (int jt = 0; jt < JT; ++jt)
#pragma unroll
        for (int r = 0; r < 4; ++r) st[(4 * fg + r) * LD2 + jt * 16 + fr] = (bf16)(dw2[ct][jt][r] * run_sc);
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
      __builtin_amdgcn_wave_barrier();
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
      if (lane < 16 * 2 * JT) {
        const int row = lane / (2 * JT), ch = lane - row * (2 * JT);
        *(u32x4*)(P2 + (size_t)(ct * 16 + row) * p.hid + j0 + jw + ch * 8) = *(const u32x4*)(st + row * LD2 + ch * 8);
      }
    }
  }
#pragma unroll
  for (int jt = 0; jt < JT; ++jt) {
    const int jb = j0 + jw + jt * 16;
    if (!part1) {
#pragma unroll
    for (int ct = 0; ct < CT16; ++ct)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        atomicAdd(&p.dw1[(long)(jb + 4 * fg + r) * C + ct * 16 + fr], dw1[jt][ct][r] * run_sc);
        atomicAdd(&p.dw2[(long)(ct * 16 + 4 * fg + r) * p.hid + jb + fr], dw2[ct][jt][r] * run_sc);
      }
    }
    if (fr == 0) {                             // every column of the ones-product holds the same sums: column 0 adds them
#pragma unroll
      for (int r = 0; r < 4; ++r) atomicAdd(&p.db1[jb + 4 * fg + r], db1m[jt][r] * run_sc);
    }
  }
  if (do_db2 && fr == 0) {
#pragma unroll
    for (int r = 0; r < 4; ++r) atomicAdd(&p.db2[wave * 16 + 4 * fg + r], db2m[r] * run_sc);
  }
}

}  // namespace

// ------------------------------------------------------------------------------------------------ plan -> launch
#define WGRAD(C) MVLT_MLP_CASE((mlp_wgrad_kernel<C>), (C), p.m_per_split, p.splits, p.ny)
#define WGRAD2(C, NW) MVLT_MLP_CASE((mlp_wgrad2_kernel<C, NW>), (C, NW), p.m_per_split, p.splits, p.ny, (void*)part1, (void*)part2)
int mvlt_launch_mlp_wgrad(const mvlt_mlp_args& a, const mvlt_mlp_plan& p, hipStream_t s, const char* who) {
  if (p.family == MVLT_MLP_WGRAD) {
    switch (mkey(p.tp[0])) {
      WGRAD(64) WGRAD(128)
      default: return mlp_no_instantiation(who, p);
    }
    return mvlt_check_launch(who);
  }
  // the token splits' partial tiles of dW1 and dW2 in the caller's scratch (ONE region for both, room for two descriptors) + two folds behind the kernel -- launched at
  // once, or appended to the scratch's pending table when the caller defers.  The plan has checked everything the bookkeeping can refuse on.
  bf16 *part1 = nullptr, *part2 = nullptr;
  mvlt_gemm_tn_args f1 = {}, f2 = {};
  if (p.fold) {
    const int C = p.tp[0];
    f1.C = a.dw1; f1.N1 = a.hid; f1.N2 = C; f1.ldc = C;
    f2.C = a.dw2; f2.N1 = C; f2.N2 = a.hid; f2.ldc = a.hid;
    f1.partials = f2.partials = a.partials; f1.partials_bytes = f2.partials_bytes = a.partials_bytes; f1.defer_fold = f2.defer_fold = a.defer_fold;
    part1 = mvlt_fold_acquire_ext(f1, p.partials_need, s, 2);
    if (!part1) { mvlt_set_error("%s: the planned %ld bytes of partial tiles do not fit the scratch", who, p.partials_need); return MVLT_ERR_ARG; }
    part2 = part1 + p.partials_need / 4;
  }
  switch (mkey(p.tp[0], p.tp[1])) {
    WGRAD2(64, 4) WGRAD2(128, 8)
    default: return mlp_no_instantiation(who, p);
  }
  if (part1) {
    mvlt_fold_launch_ext(f1, part1, p.splits, s);
    mvlt_fold_launch_ext(f2, part2, p.splits, s);
  }
  return mvlt_check_launch(who);
}

// What more than one GEMM translation unit uses (gemm.hip and one gemm_<family>.hip per kernel family; the overview is at the top of gemm.hip): tile constants,
// fragment / row-iterator / LDS-DMA helpers, the NT epilogues and, last, what the launch functions share.  Everything sits in the including file's anonymous namespace, as the
// kernels do, except the per-family launch functions, which are what gemm.hip calls across the files.
#pragma once
#include "common.h"
#include "gemm_plan.h"
#include <type_traits>
#include "../../include/mvlt_hip.h"

// One launch function per family file and entry point: the plan's (family, template arguments) -> that file's instantiation, or no_instantiation.  The TN ones get the
// kernel's view of the operands (gemm.hip has swapped them where the plan says so) and the partial-tile region of a folding plan.
int mvlt_launch_nt_dma(const mvlt_gemm_plan& p, const mvlt_gemm_nt_args& a, hipStream_t s);        // gemm_nt_dma.hip: MVLT_GEMM_NT_F32, MVLT_GEMM_NT_DMA
int mvlt_launch_nt_p8(const mvlt_gemm_plan& p, const mvlt_gemm_nt_args& a, hipStream_t s);         // gemm_nt_p8.hip
int mvlt_launch_nt_conv3(const mvlt_gemm_plan& p, const mvlt_gemm_nt_args& a, hipStream_t s);      // gemm_conv3.hip
int mvlt_launch_tn_dma(const mvlt_gemm_plan& p, const mvlt_gemm_tn_args& k, bf16* part, hipStream_t s);      // gemm_tn_dma.hip: MVLT_GEMM_TN_PLAIN, MVLT_GEMM_TN_DMA
int mvlt_launch_tn_p8(const mvlt_gemm_plan& p, const mvlt_gemm_tn_args& k, bf16* part, hipStream_t s);       // gemm_tn_p8.hip
int mvlt_launch_tn_conv3(const mvlt_gemm_plan& p, const mvlt_gemm_tn_args& k, bf16* part, hipStream_t s);    // gemm_conv3.hip

namespace {

constexpr int BM = 128;
constexpr int NTHREADS = 256;
constexpr int ROW_BYTES = 128;        // one LDS row = 128 B of K
constexpr int CHUNKS = 8;             // 16-B chunks per LDS row

template <typename T> struct Elem;
template <> struct Elem<bf16> { static constexpr int BK = 64; static constexpr int PER_CHUNK = 8; };
template <> struct Elem<float> { static constexpr int BK = 32; static constexpr int PER_CHUNK = 4; };

__device__ __forceinline__ int swz(int row, int chunk) { return chunk ^ ((row >> 1) & 7); }

__device__ __forceinline__ RowMap to_rowmap(const mvlt_rowmap& m) {
  RowMap r;
  r.mode = m.mode; r.rows_per_batch = m.rows_per_batch; r.batch_stride = m.batch_stride; r.offset = m.offset;
  r.r = m.r; r.w_in = m.w_in; r.tokens_in = m.tokens_in; r.hw_out = m.hw_out; r.w_out = m.w_out; r.c_seg = m.c_seg;
  r.h_in = m.h_in;
  return r;
}

// one k32 MFMA step on a 16x16 tile: a/b fragments = 8 consecutive K elements of row (lane&15) at K offset 8*(lane>>4)
__device__ __forceinline__ void mma16(f32x4& acc, const u32x4& a0, const u32x4& a1, const u32x4& b0, const u32x4& b1, bf16*) {
  acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, a0), __builtin_bit_cast(bf16x8, b0), acc, 0, 0, 0);
  (void)a1; (void)b1;
}
__device__ __forceinline__ void mma16(f32x4& acc, const u32x4& a0, const u32x4& a1, const u32x4& b0, const u32x4& b1, float*) {
  f32x4 fa0 = __builtin_bit_cast(f32x4, a0), fa1 = __builtin_bit_cast(f32x4, a1);
  f32x4 fb0 = __builtin_bit_cast(f32x4, b0), fb1 = __builtin_bit_cast(f32x4, b1);
#pragma unroll
  for (int j = 0; j < 4; ++j) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(fa0[j], fb0[j], acc, 0, 0, 0);
#pragma unroll
  for (int j = 0; j < 4; ++j) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(fa1[j], fb1[j], acc, 0, 0, 0);
}

// out_dtype 2 (fp16; EPI 5 only: the pre-BatchNorm conv output z, which no MFMA reads -- 11 significand bits at half the bytes of fp32, the
// reference's own autocast type for it, reference libs/vl_heads.py:15-21 under torch.cuda.amp): values saturate at the fp16 range instead of
// turning into inf, and the column statistics are taken from the ROUNDED values (mean / rstd describe z as the normalisation reads it)
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
__device__ __forceinline__ void round_f16_8(float (&v)[8]) {
#pragma unroll
  for (int e = 0; e < 8; ++e) v[e] = (float)(_Float16)__builtin_amdgcn_fmed3f(v[e], -65504.f, 65504.f);
}
template <bool NTF> __device__ __forceinline__ void store_f16_8(void* base, long ix, const float (&v)[8]) {
  f16x8 o;
#pragma unroll
  for (int e = 0; e < 8; ++e) o[e] = (_Float16)v[e];
  st_g<NTF>((f16x8*)((_Float16*)base + ix), o);
}
template <typename T> __device__ __forceinline__ void store_out(void* base, long idx, float v, int out_fp32) {
  if (out_fp32) ((float*)base)[idx] = v; else ((bf16*)base)[idx] = (bf16)v;
}
__device__ __forceinline__ float load_out(const void* base, long idx, int out_fp32) {
  return out_fp32 ? ((const float*)base)[idx] : (float)((const bf16*)base)[idx];
}

// ---------------- NT epilogue (shared by the register-staged and the LDS-DMA main loops).  Must be entered after a
// workgroup barrier that follows the last operand-tile read: the staging below reuses the tile LDS.
template <typename T, int BN>
__device__ __forceinline__ void nt_epilogue(const mvlt_gemm_nt_args& p, f32x4 (&acc)[4][BN / 32], char* smem, int m0, int n0,
                                            int wave, int lane) {
  constexpr int WN = BN / 2;
  constexpr int TN_ = WN / 16;
  const int wm = wave >> 1, wn = wave & 1;
  const int fr = lane & 15, fg = lane >> 4;
  // ---------------- epilogue: acc[i][j][r] = C[m0 + wm*64 + i*16 + 4*fg + r][n0 + wn*WN + j*16 + fr]
  // The MFMA C layout gives each lane one column and 4 rows: stored directly that is 2-byte pieces, 32 B per row.
  // Instead every wave parks its tile in the (now free) staging LDS, 32 rows at a time, and re-reads it row-major:
  // each lane then owns 8 consecutive columns of one row, so bias / GELU / residual / H traffic and the C store are
  // 16-byte accesses that cover a full 128-B (bf16) or 256-B (fp32) row segment per 8 lanes.
  const RowMap cmap = to_rowmap(p.c_map);
  const int ofp32 = p.out_dtype;
  constexpr int LDW = WN + 4;                         // fp32 words per staged row (pad: <=2-way ds_write conflicts)
  constexpr int CPR = WN / 8;                         // 8-column chunks per row
  constexpr int RPI = 64 / CPR;                       // rows covered per wave iteration
  float* stage = (float*)smem + wave * 32 * LDW;
  const bool vec_ok = (p.ldc % 8 == 0) && (((uintptr_t)p.C & 15) == 0) && (!p.R || ((uintptr_t)p.R & 15) == 0) &&
                      (!p.H || ((uintptr_t)p.H & 15) == 0);
  // this lane's 8 output columns are the same in every iteration: fetch their bias once (two 16-B loads when aligned)
  const int nc_lane = n0 + wn * WN + (lane % CPR) * 8;
  float bias8[8];
#pragma unroll
  for (int e = 0; e < 8; ++e) bias8[e] = 0.f;
  if (p.bias && p.split_k <= 1) {
    if (nc_lane + 8 <= p.N && (((uintptr_t)p.bias & 15) == 0)) {
      f32x4 b0 = *(const f32x4*)(p.bias + nc_lane), b1 = *(const f32x4*)(p.bias + nc_lane + 4);
#pragma unroll
      for (int e = 0; e < 4; ++e) { bias8[e] = b0[e]; bias8[4 + e] = b1[e]; }
    } else {
#pragma unroll
      for (int e = 0; e < 8; ++e) if (nc_lane + e < p.N) bias8[e] = p.bias[nc_lane + e];
    }
  }
  // optional per-column sum / sum of squares of the stored values (BatchNorm batch statistics of a conv output)
  float cs8[8], cq8[8];
#pragma unroll
  for (int e = 0; e < 8; ++e) { cs8[e] = 0.f; cq8[e] = 0.f; }
#pragma unroll
  // (the K loop ended with a workgroup barrier: nobody reads the operand tiles any more.  From here on every wave
  //  touches only its own staging slice, so only wave-level ordering is needed and the waves drift apart freely.)
  for (int half = 0; half < 2; ++half) {
    __builtin_amdgcn_wave_barrier();
#pragma unroll
    for (int ii = 0; ii < 2; ++ii)
#pragma unroll
      for (int j = 0; j < TN_; ++j)
#pragma unroll
        for (int r = 0; r < 4; ++r) stage[(ii * 16 + 4 * fg + r) * LDW + j * 16 + fr] = acc[half * 2 + ii][j][r];
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    if (p.split_k > 1) {
      // partial tile of a K split: fp32 atomics into the caller-zeroed C, one staged row per instruction so that the
      // lanes of a wave hit consecutive floats (whole 64-B atomic requests; the row-major 8-columns-per-lane layout
      // below would touch every request eight times)
      const int col = n0 + wn * WN + lane;
      if (lane < WN && col < p.N) {
        const float bv = (p.bias && blockIdx.y == 0) ? p.bias[col] : 0.f;
        for (int r = 0; r < 32; ++r) {
          const int m = m0 + wm * 64 + half * 32 + r;
          if (m < p.M) atomicAdd((float*)p.C + (long)m * p.ldc + col, stage[r * LDW + lane] + bv);
        }
      }
      continue;
    }
#pragma unroll
    for (int it = 0; it < 32 / RPI; ++it) {
      const int rl = it * RPI + lane / CPR;           // row inside this 32-row half
      const int ch = lane % CPR;
      const int m = m0 + wm * 64 + half * 32 + rl;
      const int nc = n0 + wn * WN + ch * 8;           // first of this lane's 8 columns
      if (m >= p.M || nc >= p.N) continue;
      f32x4 v0 = *(const f32x4*)(stage + rl * LDW + ch * 8), v1 = *(const f32x4*)(stage + rl * LDW + ch * 8 + 4);
      float v[8] = {v0[0], v0[1], v0[2], v0[3], v1[0], v1[1], v1[2], v1[3]};
      int seg_rows = 0, ncol = nc;
      if (cmap.mode == 1) {                           // scatter back through the patch map (dgrad of a kernel==stride conv)
        int seg = nc / cmap.c_seg;
        ncol = nc - seg * cmap.c_seg;
        seg_rows = rowmap_seg(cmap, seg);
      }
      const long idx = (rowmap_base(cmap, m) + seg_rows) * p.ldc + ncol;
      const bool full = vec_ok && (nc + 8 <= p.N);
      const float rs = p.row_scale ? p.row_scale[m / p.rows_per_scale] : 1.0f;
#pragma unroll
      for (int e = 0; e < 8; ++e) v[e] += bias8[e];
      if (full) {
        auto load8 = [&](const void* base, float* o) {
          if (ofp32) {
            f32x4 a = *(const f32x4*)((const float*)base + idx), b = *(const f32x4*)((const float*)base + idx + 4);
#pragma unroll
            for (int e = 0; e < 4; ++e) { o[e] = a[e]; o[4 + e] = b[e]; }
          } else {
            bf16x8 a = *(const bf16x8*)((const bf16*)base + idx);
#pragma unroll
            for (int e = 0; e < 8; ++e) o[e] = (float)a[e];
          }
        };
        auto store8 = [&](void* base, const float* o) {
          if (ofp32) {
            st_g<MVLT_NT_GEMM>((f32x4*)((float*)base + idx), f32x4{o[0], o[1], o[2], o[3]});
            st_g<MVLT_NT_GEMM>((f32x4*)((float*)base + idx + 4), f32x4{o[4], o[5], o[6], o[7]});
          } else {
            bf16x8 a;
#pragma unroll
            for (int e = 0; e < 8; ++e) a[e] = (bf16)o[e];
            st_g<MVLT_NT_GEMM>((bf16x8*)((bf16*)base + idx), a);
          }
        };
        if (p.act == 1) {
          if (p.H) store8(p.H, v);
#pragma unroll
          for (int e = 0; e < 8; e += 2) {
            const f32x2 gv = gelu_erf2(f32x2{v[e], v[e + 1]});
            v[e] = gv[0]; v[e + 1] = gv[1];
          }
        } else if (p.act == 2) {
          float h8[8];
          load8(p.H, h8);
#pragma unroll
          for (int e = 0; e < 8; e += 2) {
            const f32x2 dv = gelu_erf_grad2(f32x2{h8[e], h8[e + 1]});
            v[e] *= dv[0]; v[e + 1] *= dv[1];
          }
        }
        if (p.row_scale) {
#pragma unroll
          for (int e = 0; e < 8; ++e) v[e] *= rs;
        }
        if (p.R) {
          float r8[8];
          load8(p.R, r8);
#pragma unroll
          for (int e = 0; e < 8; ++e) v[e] += r8[e];
        }
        if (p.col_sum) {
#pragma unroll
          for (int e = 0; e < 8; ++e) { cs8[e] += v[e]; cq8[e] += v[e] * v[e]; }
        }
        store8(p.C, v);
      } else {                                        // ragged N (vocabulary tail, 2/48/122-way heads) or unaligned rows
        for (int e = 0; e < 8; ++e) {
          if (nc + e >= p.N) break;
          float x = v[e];
          if (p.act == 1) {
            if (p.H) store_out<T>(p.H, idx + e, x, ofp32);
            x = gelu_erf(x);
          } else if (p.act == 2) {
            x *= gelu_erf_grad(load_out(p.H, idx + e, ofp32));
          }
          x *= rs;
          if (p.R) x += load_out(p.R, idx + e, ofp32);
          if (p.col_sum) { cs8[e] += x; cq8[e] += x * x; }
          store_out<T>(p.C, idx + e, x, ofp32);
        }
      }
    }
  }
  if (p.col_sum) {
    // lanes with equal lane % CPR own the same 8 columns: fold them, then turn the CPR x 8 totals of this wave into one
    // 64-lane (32 for the narrow tile) atomic per statistic through the wave's staging slice
#pragma unroll
    for (int off = CPR; off < 64; off <<= 1)
#pragma unroll
      for (int e = 0; e < 8; ++e) { cs8[e] += __shfl_xor(cs8[e], off); cq8[e] += __shfl_xor(cq8[e], off); }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    if (lane < CPR) {
#pragma unroll
      for (int e = 0; e < 8; ++e) { stage[lane * 8 + e] = cs8[e]; stage[WN + lane * 8 + e] = cq8[e]; }
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    // every row tile of the launch adds into the same N floats; same-line atomics serialise at the memory side, so the
    // caller provides col_copies interleaved accumulators ([copy][N]) and sums them when it finalises the statistics
    const int col = n0 + wn * WN + lane;
    const long cpy = p.col_copies > 1 ? (long)((m0 / BM) % p.col_copies) * p.N : 0;
    if (lane < WN && col < p.N) {
      atomicAdd(&p.col_sum[cpy + col], stage[lane]);
      atomicAdd(&p.col_sumsq[cpy + col], stage[WN + lane]);
    }
  }
}

// ---------------- lean NT epilogues (bf16 LDS-DMA kernels).  The generic epilogue above decides every feature at run time
// inside the per-row loop and recomputes row / column addressing per 8 outputs: ~100 instructions per 8 outputs, 55 % of
// the stage-3 fc1 GEMM's time.  The call sites use five shapes of epilogue; each gets a compile-time variant in which the
// column side (bias, chunk index) is fixed per lane, the row side is a multiply, and the operands a variant needs (R, H,
// DropPath factor) are requested for a whole 32-row half before it is processed.  Preconditions (checked by the host
// dispatch): identity, batch-strided or patch-scatter c_map, N % 8 == 0, ldc % 8 == 0, 16-byte aligned C / R / H, no split-K.
//   EPI 1: C = AB^T (+bias)                      EPI 2: C = (AB^T + bias) * row_scale + R
//   EPI 3: H = AB^T + bias ; C = gelu(H)         EPI 4: C = AB^T * gelu'(H)          EPI 5: EPI 1 + column sum / sum of squares
//   EPI 6 / 7: EPI 1 / 2 written through a patch-scatter c_map (dgrad of the kernel==stride convs)
//   EPI 8: EPI 2 + LayerNorm of the finished row (N == BN: the tile holds whole rows, split over the two waves of a row pair):
//          post_y = LN(C row; post_gamma, post_beta, post_eps) in bf16 + the row statistics -- Block.norm2 behind attn.proj
//          (reference libs/pvlt.py:140-142) without a pass of its own over the fp32 mid stream
__device__ __forceinline__ int fdiv24(int m, int d, float inv) {      // exact m / d for 0 <= m < 2^24, inv = 1.0f / d
  int q = (int)((float)m * inv);
  int r = m - q * d;
  return q + (r >= d) - (r < 0);
}
// NWN = waves along N (2: the 4-wave 2 x 2 kernels; 4: the 8-wave 256 x 256 kernel, whose wave tile is (TM * 16) x 64 = "BN 128" here)
// FULL: the launch has whole tiles only (no row / column bound checks: the 8-wave kernels, whose epilogue is issue-bound at two waves per SIMD)
template <int BN, int EPIX, int TM = 4, int NWN = 2, bool FULL = false>
__device__ __forceinline__ void nt_epilogue_lean(const mvlt_gemm_nt_args& p, f32x4 (&acc)[TM][BN / 32], char* smem, int m0, int n0,
                                                 int wave, int lane) {
  static_assert(NWN == 2 || EPIX != 8, "the LayerNorm epilogue pairs the two waves of a row: 2 x 2 wave grids only");
  constexpr bool SCAT = (EPIX == 6 || EPIX == 7);     // EPI 6 / 7 = EPI 1 / 2 with a patch-scatter c_map (mode 1)
  constexpr bool POST = EPIX == 8;                    // EPI 8 = EPI 2 + LayerNorm of the output row
  constexpr int EPI = EPIX == 6 ? 1 : (EPIX == 7 || EPIX == 8) ? 2 : EPIX;
  constexpr int WN = BN / 2;
  constexpr int TN_ = WN / 16;
  constexpr int LDW = WN + 4;
  constexpr int CPR = WN / 8;
  constexpr int RPI = 64 / CPR;
  constexpr int NIT = 32 / RPI;
  const int wm = wave / NWN, wn = wave % NWN;
  const int fr = lane & 15, fg = lane >> 4;
  // the GELU / GELU' epilogues write (and read) operand-dtype tensors only -- the host dispatch guarantees it -- so their fp32 store / load
  // paths and the second half of every prefetch slot are not compiled in (EPI 4: 119 -> fewer registers, a third workgroup per CU)
  const int ofp32 = (EPI == 3 || EPI == 4) ? 0 : p.out_dtype;
  const int rfp32 = (EPI == 2 && !POST) ? (ofp32 | p.r_fp32) : ofp32;      // EPI 2: the residual may be fp32 beside a bf16 C (mvlt_gemm_nt_args.r_fp32)
  float* stage = (float*)smem + wave * 32 * LDW;
  const int ch = lane % CPR;
  const int nc = n0 + wn * WN + ch * 8;
  const bool col_ok = FULL || nc < p.N;
  float bias8[8];
#pragma unroll
  for (int e = 0; e < 8; ++e) bias8[e] = 0.f;
  if (p.bias && col_ok) {
    if (!FULL && nc + 8 > p.N) {                       // the last, partial chunk of a row whose length is not a multiple of 8 (EPI 1 only: host dispatch)
#pragma unroll
      for (int e = 0; e < 8; ++e) if (nc + e < p.N) bias8[e] = p.bias[nc + e];
    } else if (((uintptr_t)p.bias & 15) == 0) {
      f32x4 b0 = *(const f32x4*)(p.bias + nc), b1 = *(const f32x4*)(p.bias + nc + 4);
#pragma unroll
      for (int e = 0; e < 4; ++e) { bias8[e] = b0[e]; bias8[4 + e] = b1[e]; }
    } else {
#pragma unroll
      for (int e = 0; e < 8; ++e) bias8[e] = p.bias[nc + e];
    }
  }
  constexpr int NH = TM / 2;                          // 32-row halves of the wave tile (2, or 4 under the 256-row tile)
  const int m_first = m0 + wm * (TM * 16) + lane / CPR;
  const int rpb = p.c_map.rows_per_batch;
  const float inv_rpb = rpb > 0 ? 1.0f / (float)rpb : 0.f;
  // patch scatter (c_map mode 1, dgrad of a kernel==stride conv): this lane's 8 columns lie in one (di, dj) segment
  int seg_rows = 0, ncol = nc;
  float inv_hw = 0.f, inv_w = 0.f;
  if constexpr (SCAT) {
    const int seg = nc / p.c_map.c_seg;
    ncol = nc - seg * p.c_map.c_seg;
    const int di = seg / p.c_map.r;
    seg_rows = di * p.c_map.w_in + (seg - di * p.c_map.r);
    inv_hw = 1.0f / (float)p.c_map.hw_out;
    inv_w = 1.0f / (float)p.c_map.w_out;
  }
  const float inv_rps = (EPI == 2 && p.rows_per_scale > 0) ? 1.0f / (float)p.rows_per_scale : 0.f;
  float cs8[8], cq8[8];
  if (EPI == 5) {
#pragma unroll
    for (int e = 0; e < 8; ++e) { cs8[e] = 0.f; cq8[e] = 0.f; }
  }
  // R (EPI 2) / H (EPI 4) of two 32-row halves are requested before the first one is staged (two rotating slots): their HBM
  // latency hides behind the LDS staging and the previous half instead of being paid once per half
  long idx[2][NIT];
  bool ok[2][NIT];
  float rs[2][NIT];
  u32x4 raw[2][NIT][2];
  auto request = [&](int half) {
    const int sl = half & 1;
#pragma unroll
    for (int it = 0; it < NIT; ++it) {
      const int m = m_first + half * 32 + it * RPI;
      ok[sl][it] = FULL || (m < p.M && col_ok);
      const int mm = (FULL || ok[sl][it]) ? m : 0;
      long phys = mm;
      if constexpr (SCAT) {
        const int b = fdiv24(mm, p.c_map.hw_out, inv_hw);
        const int rem = mm - b * p.c_map.hw_out;
        const int oi = fdiv24(rem, p.c_map.w_out, inv_w), oj = rem - oi * p.c_map.w_out;
        phys = (long)b * p.c_map.tokens_in + (long)(oi * p.c_map.r) * p.c_map.w_in + oj * p.c_map.r + seg_rows;
      } else if (rpb > 0) {
        const int b = fdiv24(mm, rpb, inv_rpb);
        phys = (long)b * p.c_map.batch_stride + p.c_map.offset + (mm - b * rpb);
      }
      idx[sl][it] = phys * p.ldc + ncol;
      rs[sl][it] = 1.0f;
      if (EPI == 2 && p.row_scale) rs[sl][it] = p.row_scale[fdiv24(mm, p.rows_per_scale, inv_rps)];
      if ((EPI == 2 || EPI == 4) && (FULL || ok[sl][it])) {
        const void* src = (EPI == 2) ? p.R : p.H;
        if (rfp32) { raw[sl][it][0] = ld_g<MVLT_NT_LD>((const u32x4*)((const float*)src + idx[sl][it])); raw[sl][it][1] = ld_g<MVLT_NT_LD>((const u32x4*)((const float*)src + idx[sl][it] + 4)); }
        else raw[sl][it][0] = ld_g<MVLT_NT_LD>((const u32x4*)((const bf16*)src + idx[sl][it]));
      }
    }
  };
  constexpr bool PREFETCH = (EPI == 2 || EPI == 4);
  if (PREFETCH) { request(0); request(1); }
  float pgam[8], pbet[8];
  float* const xch = (float*)smem + 4 * 32 * LDW;    // POST: [128 rows][2 column halves] row sums | the same for the squared deviations
  if constexpr (POST) {
#pragma unroll
    for (int e = 0; e < 8; ++e) { pgam[e] = p.post_gamma[nc + e]; pbet[e] = p.post_beta[nc + e]; }
  }
#pragma unroll
  for (int half = 0; half < NH; ++half) {
    const int sl = half & 1;
    __builtin_amdgcn_wave_barrier();
#pragma unroll
    for (int ii = 0; ii < 2; ++ii)
#pragma unroll
      for (int j = 0; j < TN_; ++j)
#pragma unroll
        for (int r = 0; r < 4; ++r) stage[(ii * 16 + 4 * fg + r) * LDW + j * 16 + fr] = acc[half * 2 + ii][j][r];
    if (!PREFETCH) request(half);
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    if constexpr (POST) {
      // the row's other half lives in the partner wave (wn ^ 1): two-pass statistics with one LDS exchange + workgroup barrier per pass
      const float inv_n = 1.0f / (float)p.N;
      float keep[NIT][8];
#pragma unroll
      for (int it = 0; it < NIT; ++it) {
        const int rl = it * RPI + lane / CPR;
        float sum = 0.f;
#pragma unroll
        for (int e = 0; e < 8; ++e) keep[it][e] = 0.f;
        if (ok[sl][it]) {
          const f32x4 v0 = *(const f32x4*)(stage + rl * LDW + ch * 8), v1 = *(const f32x4*)(stage + rl * LDW + ch * 8 + 4);
          float v[8] = {v0[0], v0[1], v0[2], v0[3], v1[0], v1[1], v1[2], v1[3]};
          float o8[8];
          if (ofp32) {
            const f32x4 a = __builtin_bit_cast(f32x4, raw[sl][it][0]), b = __builtin_bit_cast(f32x4, raw[sl][it][1]);
#pragma unroll
            for (int e = 0; e < 4; ++e) { o8[e] = a[e]; o8[4 + e] = b[e]; }
          } else {
            const bf16x8 a = __builtin_bit_cast(bf16x8, raw[sl][it][0]);
#pragma unroll
            for (int e = 0; e < 8; ++e) o8[e] = (float)a[e];
          }
#pragma unroll
          for (int e = 0; e < 8; ++e) { v[e] = (v[e] + bias8[e]) * rs[sl][it] + o8[e]; keep[it][e] = v[e]; sum += v[e]; }
          const long ix = idx[sl][it];
          if (ofp32) {
            st_g<MVLT_NT_GEMM>((f32x4*)((float*)p.C + ix), f32x4{v[0], v[1], v[2], v[3]});
            st_g<MVLT_NT_GEMM>((f32x4*)((float*)p.C + ix + 4), f32x4{v[4], v[5], v[6], v[7]});
          } else {
            bf16x8 a;
#pragma unroll
            for (int e = 0; e < 8; ++e) a[e] = (bf16)v[e];
            st_g<MVLT_NT_GEMM>((bf16x8*)((bf16*)p.C + ix), a);
          }
        }
#pragma unroll
        for (int o = 1; o < CPR; o <<= 1) sum += __shfl_xor(sum, o);
        if (ch == 0) xch[((wm * 2 + half) * 32 + rl) * 2 + wn] = sum;
      }
      __syncthreads();
      float mean[NIT];
#pragma unroll
      for (int it = 0; it < NIT; ++it) {
        const int row = (wm * 2 + half) * 32 + it * RPI + lane / CPR;
        mean[it] = (xch[row * 2] + xch[row * 2 + 1]) * inv_n;
        float q = 0.f;
#pragma unroll
        for (int e = 0; e < 8; ++e) { keep[it][e] -= mean[it]; q += keep[it][e] * keep[it][e]; }
#pragma unroll
        for (int o = 1; o < CPR; o <<= 1) q += __shfl_xor(q, o);
        if (ch == 0) xch[256 + row * 2 + wn] = q;
      }
      __syncthreads();
#pragma unroll
      for (int it = 0; it < NIT; ++it) {
        if (!ok[sl][it]) continue;
        const int rl = it * RPI + lane / CPR;
        const int row = (wm * 2 + half) * 32 + rl;
        const int m = m_first + half * 32 + it * RPI;
        const float rstd = rsqrtf((xch[256 + row * 2] + xch[256 + row * 2 + 1]) * inv_n + p.post_eps);
        bf16x8 y;
#pragma unroll
        for (int e = 0; e < 8; ++e) y[e] = (bf16)(keep[it][e] * rstd * pgam[e] + pbet[e]);
        st_g<MVLT_NT_GEMM>((bf16x8*)((bf16*)p.post_y + (long)m * p.post_ld + nc), y);
        if (wn == 0 && ch == 0) { p.post_mean[m] = mean[it]; p.post_rstd[m] = rstd; }
      }
      if (PREFETCH && half + 2 < NH) request(half + 2);
      continue;
    }
#pragma unroll
    for (int it = 0; it < NIT; ++it) {
      if (!FULL && !ok[sl][it]) continue;
      const int rl = it * RPI + lane / CPR;
      const f32x4 v0 = *(const f32x4*)(stage + rl * LDW + ch * 8), v1 = *(const f32x4*)(stage + rl * LDW + ch * 8 + 4);
      float v[8] = {v0[0], v0[1], v0[2], v0[3], v1[0], v1[1], v1[2], v1[3]};
#pragma unroll
      for (int e = 0; e < 8; ++e) v[e] += bias8[e];
      const long ix = idx[sl][it];
      auto store8 = [&](void* base, const float* o) {
        if (EPI == 5 && ofp32 == 2) {
          const float o8h[8] = {o[0], o[1], o[2], o[3], o[4], o[5], o[6], o[7]};
          store_f16_8<MVLT_NT_GEMM>(base, ix, o8h);
        } else if (ofp32) {
          st_g<MVLT_NT_GEMM>((f32x4*)((float*)base + ix), f32x4{o[0], o[1], o[2], o[3]});
          st_g<MVLT_NT_GEMM>((f32x4*)((float*)base + ix + 4), f32x4{o[4], o[5], o[6], o[7]});
        } else {
          bf16x8 a;
#pragma unroll
          for (int e = 0; e < 8; ++e) a[e] = (bf16)o[e];
          st_g<MVLT_NT_GEMM>((bf16x8*)((bf16*)base + ix), a);
        }
      };
      float o8[8];
      if (EPI == 2 || EPI == 4) {
        if (rfp32) {
          const f32x4 a = __builtin_bit_cast(f32x4, raw[sl][it][0]), b = __builtin_bit_cast(f32x4, raw[sl][it][1]);
#pragma unroll
          for (int e = 0; e < 4; ++e) { o8[e] = a[e]; o8[4 + e] = b[e]; }
        } else {
          const bf16x8 a = __builtin_bit_cast(bf16x8, raw[sl][it][0]);
#pragma unroll
          for (int e = 0; e < 8; ++e) o8[e] = (float)a[e];
        }
      }
      if (EPI == 3) {
        if (p.H) store8(p.H, v);
#pragma unroll
        for (int e = 0; e < 8; e += 2) {
          const f32x2 gv = gelu_fast2(f32x2{v[e], v[e + 1]});
          v[e] = gv[0]; v[e + 1] = gv[1];
        }
      }
      if (EPI == 4) {
#pragma unroll
        for (int e = 0; e < 8; e += 2) {
          const f32x2 dv = gelu_fast_grad2(f32x2{o8[e], o8[e + 1]});
          v[e] *= dv[0]; v[e + 1] *= dv[1];
        }
      }
      if (EPI == 2) {
#pragma unroll
        for (int e = 0; e < 8; ++e) v[e] = v[e] * rs[sl][it] + o8[e];
      }
      if (EPI == 5) {
        if (ofp32 == 2) round_f16_8(v);
#pragma unroll
        for (int e = 0; e < 8; ++e) { cs8[e] += v[e]; cq8[e] += v[e] * v[e]; }
      }
      if constexpr (EPI == 1 && !FULL && !SCAT) {
        if (nc + 8 > p.N) {                            // partial last chunk: its valid columns one by one, nothing past column N - 1 is touched
#pragma unroll
          for (int e = 0; e < 8; ++e)
            if (nc + e < p.N) { if (ofp32) ((float*)p.C)[ix + e] = v[e]; else ((bf16*)p.C)[ix + e] = (bf16)v[e]; }
          continue;
        }
      }
      store8(p.C, v);
    }
    if (PREFETCH && half + 2 < NH) request(half + 2);
  }
  if (EPI == 5) {
#pragma unroll
    for (int off = CPR; off < 64; off <<= 1)
#pragma unroll
      for (int e = 0; e < 8; ++e) { cs8[e] += __shfl_xor(cs8[e], off); cq8[e] += __shfl_xor(cq8[e], off); }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    if (lane < CPR) {
#pragma unroll
      for (int e = 0; e < 8; ++e) { stage[lane * 8 + e] = cs8[e]; stage[WN + lane * 8 + e] = cq8[e]; }
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    const int col = n0 + wn * WN + lane;
    const long cpy = p.col_copies > 1 ? (long)((m0 / BM) % p.col_copies) * p.N : 0;
    if (lane < WN && col < p.N) {
      atomicAdd(&p.col_sum[cpy + col], stage[lane]);
      atomicAdd(&p.col_sumsq[cpy + col], stage[WN + lane]);
    }
  }
}

// BN = 192 (wave tile 64 x 96, for N % 192 == 0 outputs that the 128-wide tile would pad to the next 256): the wave's 96 columns
// leave as three 32-column groups, 4 lanes x 8 columns per row and 16 rows per instruction.  Only the two epilogues the
// 192-channel convolutions use: EPI 1 (plain (+bias)) and EPI 5 (the same + column sum / sum of squares).
template <int EPI>
__device__ __forceinline__ void nt_epilogue_192(const mvlt_gemm_nt_args& p, f32x4 (&acc)[4][6], char* smem, int m0, int n0, int wave,
                                                int lane) {
  static_assert(EPI == 1 || EPI == 5, "192-wide tiles carry the plain and the column-statistics epilogue only");
  constexpr int WN = 96, TN_ = 6, LDW = WN + 4, NG = 3;
  const int wm = wave >> 1, wn = wave & 1;
  const int fr = lane & 15, fg = lane >> 4;
  const int ofp32 = p.out_dtype;
  float* stage = (float*)smem + wave * 32 * LDW;
  const int ch = lane & 3, rl0 = lane >> 2;
  const int nbase = n0 + wn * WN + ch * 8;
  const int rpb = p.c_map.rows_per_batch;
  const float inv_rpb = rpb > 0 ? 1.0f / (float)rpb : 0.f;
  float cs[NG][8], cq[NG][8];
  if (EPI == 5) {
#pragma unroll
    for (int g = 0; g < NG; ++g)
#pragma unroll
      for (int e = 0; e < 8; ++e) { cs[g][e] = 0.f; cq[g][e] = 0.f; }
  }
#pragma unroll
  for (int half = 0; half < 2; ++half) {
    __builtin_amdgcn_wave_barrier();
#pragma unroll
    for (int ii = 0; ii < 2; ++ii)
#pragma unroll
      for (int j = 0; j < TN_; ++j)
#pragma unroll
        for (int r = 0; r < 4; ++r) stage[(ii * 16 + 4 * fg + r) * LDW + j * 16 + fr] = acc[half * 2 + ii][j][r];
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
#pragma unroll
    for (int it = 0; it < 2; ++it) {
      const int rl = it * 16 + rl0;
      const int m = m0 + wm * 64 + half * 32 + rl;
      if (m >= p.M) continue;
      long phys = m;
      if (rpb > 0) {
        const int b = fdiv24(m, rpb, inv_rpb);
        phys = (long)b * p.c_map.batch_stride + p.c_map.offset + (m - b * rpb);
      }
#pragma unroll
      for (int g = 0; g < NG; ++g) {
        const int nc = nbase + g * 32;
        if (nc >= p.N) continue;
        const f32x4 v0 = *(const f32x4*)(stage + rl * LDW + g * 32 + ch * 8), v1 = *(const f32x4*)(stage + rl * LDW + g * 32 + ch * 8 + 4);
        float v[8] = {v0[0], v0[1], v0[2], v0[3], v1[0], v1[1], v1[2], v1[3]};
        if (p.bias) {
#pragma unroll
          for (int e = 0; e < 8; ++e) v[e] += p.bias[nc + e];
        }
        if (EPI == 5) {
          if (ofp32 == 2) round_f16_8(v);
#pragma unroll
          for (int e = 0; e < 8; ++e) { cs[g][e] += v[e]; cq[g][e] += v[e] * v[e]; }
        }
        const long ix = phys * p.ldc + nc;
        if (EPI == 5 && ofp32 == 2) {
          store_f16_8<MVLT_NT_GEMM>(p.C, ix, v);
        } else if (ofp32) {
          st_g<MVLT_NT_GEMM>((f32x4*)((float*)p.C + ix), f32x4{v[0], v[1], v[2], v[3]});
          st_g<MVLT_NT_GEMM>((f32x4*)((float*)p.C + ix + 4), f32x4{v[4], v[5], v[6], v[7]});
        } else {
          bf16x8 o;
#pragma unroll
          for (int e = 0; e < 8; ++e) o[e] = (bf16)v[e];
          st_g<MVLT_NT_GEMM>((bf16x8*)((bf16*)p.C + ix), o);
        }
      }
    }
  }
  if (EPI == 5) {
#pragma unroll
    for (int off = 4; off < 64; off <<= 1)
#pragma unroll
      for (int g = 0; g < NG; ++g)
#pragma unroll
        for (int e = 0; e < 8; ++e) { cs[g][e] += __shfl_xor(cs[g][e], off); cq[g][e] += __shfl_xor(cq[g][e], off); }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    if (lane < 4) {
#pragma unroll
      for (int g = 0; g < NG; ++g)
#pragma unroll
        for (int e = 0; e < 8; ++e) { stage[g * 32 + lane * 8 + e] = cs[g][e]; stage[WN + g * 32 + lane * 8 + e] = cq[g][e]; }
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    const long cpy = p.col_copies > 1 ? (long)((m0 / BM) % p.col_copies) * p.N : 0;
    for (int c = lane; c < WN; c += 64) {
      const int col = n0 + wn * WN + c;
      if (col < p.N) {
        atomicAdd(&p.col_sum[cpy + col], stage[c]);
        atomicAdd(&p.col_sumsq[cpy + col], stage[WN + c]);
      }
    }
  }
}

// ---------------- TN tiles: m per LDS tile, row pitch of the transposed (register-staged) tiles
constexpr int TBK = 64;                         // m per LDS tile (both dtypes)
template <typename T> struct TElem;
template <> struct TElem<bf16> { static constexpr int ROWB = (TBK + 8) * 2; };     // 144 B rows (pad keeps 16-B alignment)
template <> struct TElem<float> { static constexpr int ROWB = (TBK + 4) * 4; };    // 272 B rows

// Logical row m of a row map as (b, y, x) digits, advanced by a fixed stride with carries instead of divisions: the
// loader of a thread visits rows m0, m0+64, m0+128, ... and one division per row would cost more than the MFMAs it
// feeds.  plain rows: x = m; batch-strided rows: (b, x) base rows_per_batch; patch / 3x3 maps: (b, y, x) in the
// output grid.
struct RowIt { int b, y, x; };
struct RowStep { int w, h, db, dy, dx; };
__device__ __forceinline__ RowStep row_step(const RowMap& rm, int delta) {
  RowStep s;
  if (rm.mode == 0) {
    if (rm.rows_per_batch == 0) { s.w = 0x7fffffff; s.h = 1; s.db = 0; s.dy = 0; s.dx = delta; }
    else { s.w = rm.rows_per_batch; s.h = 1; s.db = delta / s.w; s.dy = 0; s.dx = delta - s.db * s.w; }
  } else {
    s.w = rm.w_out; s.h = rm.hw_out / rm.w_out;
    s.db = delta / rm.hw_out;
    int rem = delta - s.db * rm.hw_out;
    s.dy = rem / s.w; s.dx = rem - s.dy * s.w;
  }
  return s;
}
__device__ __forceinline__ RowIt row_init(const RowMap& rm, int m) {
  RowIt it;
  if (rm.mode == 0) {
    if (rm.rows_per_batch == 0) { it.b = 0; it.y = 0; it.x = m; }
    else { it.b = m / rm.rows_per_batch; it.y = 0; it.x = m - it.b * rm.rows_per_batch; }
  } else {
    it.b = m / rm.hw_out;
    int rem = m - it.b * rm.hw_out;
    it.y = rem / rm.w_out; it.x = rem - it.y * rm.w_out;
  }
  return it;
}
__device__ __forceinline__ void row_advance(RowIt& it, const RowStep& s) {
  it.x += s.dx;
  int c = it.x >= s.w;
  it.x -= c ? s.w : 0;
  it.y += s.dy + c;
  int c2 = it.y >= s.h;
  it.y -= c2 ? s.h : 0;
  it.b += s.db + c2;
}
// physical row for the thread's column segment (tap dy,dx for the 3x3 map; seg_rows for the patch map); false = zero.
// MODE is a template parameter so that the per-tile loader has no mode branches (plain rows are mode 0 with b = 0).
template <int MODE>
__device__ __forceinline__ bool row_phys(const RowMap& rm, const RowIt& it, int tap_dy, int tap_dx, int seg_rows, int& phys) {
  if constexpr (MODE == 0) {
    phys = it.b * rm.batch_stride + rm.offset + it.x;
    return true;
  } else if constexpr (MODE == 1) {
    phys = it.b * rm.tokens_in + (it.y * rm.r) * rm.w_in + it.x * rm.r + seg_rows;
    return true;
  } else {
    int y = it.y + tap_dy, x = it.x + tap_dx;
    phys = it.b * rm.tokens_in + y * rm.w_in + x;
    return (unsigned)y < (unsigned)rm.h_in && (unsigned)x < (unsigned)rm.w_in;
  }
}

// geometry of one [64 m][W n] bf16 tile (W = 128 or 64): 16-B slots per row, rows per 256-thread pass, bank hash
template <int W> struct DmaTile {
  static constexpr int CH = W / 8, RPP = NTHREADS / CH, IT = TBK / RPP, ROWB = W * 2, BYTES = TBK * ROWB;
  // 256-B rows (W=128): rows m..m+3, m+8..m+11 of a read group all start on bank 0 -> spread by (m&3, bit 3);
  // 128-B rows (W=64): bit 0 of the row already picks the bank half -> spread by (bit 1, bit 3)
  static __device__ __forceinline__ int h(int row) {
    return W == 128 ? ((row & 3) | (((row >> 3) & 1) << 2)) : (((row >> 1) & 1) | (((row >> 3) & 1) << 1));
  }
  static __device__ __forceinline__ int frag_off(int frow, int window, int L) {
    return frow * ROWB + ((window ^ h(frow)) << 5) + ((L & 3) << 3);
  }
};

// ---------------- 8-wave / 8-phase kernels (gemm_nt_p8.hip, gemm_tn_p8.hip): LDS-DMA from a scalar base, scheduling fences, counted waits
__device__ __forceinline__ void glds16_s(const char* sbase, unsigned voff, unsigned dst) {
  unsigned keep;
  asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %3\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, %2\n\ts_mov_b32 m0, %0"
               : "=&s"(keep) : "v"(voff), "s"(sbase), "s"(dst) : "memory");
}
#define MVLT_BAR()                                  \
  do {                                              \
    __builtin_amdgcn_sched_barrier(0);              \
    __builtin_amdgcn_s_barrier();                   \
    asm volatile("" ::: "memory");                  \
    __builtin_amdgcn_sched_barrier(0);              \
  } while (0)
template <int N> __device__ __forceinline__ void wait_vm() { asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N) : "memory"); }
template <int N> __device__ __forceinline__ void wait_lgkm() { asm volatile("s_waitcnt lgkmcnt(%0)" ::"n"(N) : "memory"); }

// epilogue of the 80-column wave tile (BN 320 = 4 waves x 5 accumulator tiles): a 32-row half of the wave tile is 32 x 10 chunks of 8 columns =
// 5 chunks per lane.  EPI 1: C = AB^T (+bias); EPI 2: C = (AB^T + bias) * row_scale + R.  Identity or batch-strided c_map, fp32 / bf16 output.
// CHK (round 6): the last row tile is ragged (M % 192 != 0: pvlt_medium at 384 px has 45056 rows per stage-3 launch) -- requests are clamped to the last row, rows past M are not stored.
template <int EPI, int TM, bool CHK = false>
__device__ __forceinline__ void nt_epilogue_w80(const mvlt_gemm_nt_args& p, f32x4 (&acc)[TM][5], char* smem, int m0, int n0, int wave, int lane) {
  static_assert(EPI == 1 || EPI == 2, "the 80-column wave tile carries the plain and the residual epilogue");
  constexpr int WN = 80, LDW = WN + 4, NH = TM / 2, NIT = 5;
  const int wm = wave >> 2, wn = wave & 3;
  const int fr = lane & 15, fg = lane >> 4;
  const int ofp32 = p.out_dtype;
  const int rfp32 = ofp32 | p.r_fp32;                  // the residual may be fp32 beside a bf16 C (mvlt_gemm_nt_args.r_fp32)
  float* stage = (float*)smem + wave * 32 * LDW;
  const int rpb = p.c_map.rows_per_batch;
  const float inv_rpb = rpb > 0 ? 1.0f / (float)rpb : 0.f;
  const float inv_rps = (EPI == 2 && p.rows_per_scale > 0) ? 1.0f / (float)p.rows_per_scale : 0.f;
  int rl[NIT], cc[NIT];
#pragma unroll
  for (int it = 0; it < NIT; ++it) {
    const int sidx = it * 64 + lane;
    rl[it] = sidx / 10;
    cc[it] = (sidx - rl[it] * 10) * 8;
  }
  // the residual rows (EPI 2) of a 32-row half are requested one half ahead, in two rotating slots: their HBM latency hides behind the
  // previous half's staging, arithmetic and stores (the fragment registers of the K-loop are dead here)
  long idx[2][NIT];
  float rs[2][NIT];
  u32x4 raw[2][NIT][2];
  auto request = [&](int half) {
    const int sl = half & 1;
#pragma unroll
    for (int it = 0; it < NIT; ++it) {
      const int m = CHK ? min(m0 + wm * (TM * 16) + half * 32 + rl[it], p.M - 1) : m0 + wm * (TM * 16) + half * 32 + rl[it];
      long phys = m;
      if (rpb > 0) {
        const int b = fdiv24(m, rpb, inv_rpb);
        phys = (long)b * p.c_map.batch_stride + p.c_map.offset + (m - b * rpb);
      }
      idx[sl][it] = phys * p.ldc + n0 + wn * WN + cc[it];
      rs[sl][it] = 1.0f;
      if (EPI == 2) {
        if (p.row_scale) rs[sl][it] = p.row_scale[fdiv24(m, p.rows_per_scale, inv_rps)];
        if (rfp32) { raw[sl][it][0] = ld_g<MVLT_NT_LD>((const u32x4*)((const float*)p.R + idx[sl][it])); raw[sl][it][1] = ld_g<MVLT_NT_LD>((const u32x4*)((const float*)p.R + idx[sl][it] + 4)); }
        else raw[sl][it][0] = ld_g<MVLT_NT_LD>((const u32x4*)((const bf16*)p.R + idx[sl][it]));
      }
    }
  };
  request(0);
#pragma unroll
  for (int half = 0; half < NH; ++half) {
    const int sl = half & 1;
    __builtin_amdgcn_wave_barrier();
#pragma unroll
    for (int ii = 0; ii < 2; ++ii)
#pragma unroll
      for (int j = 0; j < 5; ++j)
#pragma unroll
        for (int r = 0; r < 4; ++r) stage[(ii * 16 + 4 * fg + r) * LDW + j * 16 + fr] = acc[half * 2 + ii][j][r];
    if (half + 1 < NH) request(half + 1);
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
#pragma unroll
    for (int it = 0; it < NIT; ++it) {
      if (CHK && m0 + wm * (TM * 16) + half * 32 + rl[it] >= p.M) continue;
      const f32x4 v0 = *(const f32x4*)(stage + rl[it] * LDW + cc[it]), v1 = *(const f32x4*)(stage + rl[it] * LDW + cc[it] + 4);
      float v[8] = {v0[0], v0[1], v0[2], v0[3], v1[0], v1[1], v1[2], v1[3]};
      if (p.bias) {
        const f32x4 b0 = *(const f32x4*)(p.bias + n0 + wn * WN + cc[it]), b1 = *(const f32x4*)(p.bias + n0 + wn * WN + cc[it] + 4);
#pragma unroll
        for (int e = 0; e < 4; ++e) { v[e] += b0[e]; v[4 + e] += b1[e]; }
      }
      if (EPI == 2) {
        float o8[8];
        if (rfp32) {
          const f32x4 a = __builtin_bit_cast(f32x4, raw[sl][it][0]), b = __builtin_bit_cast(f32x4, raw[sl][it][1]);
#pragma unroll
          for (int e = 0; e < 4; ++e) { o8[e] = a[e]; o8[4 + e] = b[e]; }
        } else {
          const bf16x8 a = __builtin_bit_cast(bf16x8, raw[sl][it][0]);
#pragma unroll
          for (int e = 0; e < 8; ++e) o8[e] = (float)a[e];
        }
#pragma unroll
        for (int e = 0; e < 8; ++e) v[e] = v[e] * rs[sl][it] + o8[e];
      }
      if (ofp32) {
        st_g<MVLT_NT_GEMM>((f32x4*)((float*)p.C + idx[sl][it]), f32x4{v[0], v[1], v[2], v[3]});
        st_g<MVLT_NT_GEMM>((f32x4*)((float*)p.C + idx[sl][it] + 4), f32x4{v[4], v[5], v[6], v[7]});
      } else {
        bf16x8 a;
#pragma unroll
        for (int e = 0; e < 8; ++e) a[e] = (bf16)v[e];
        st_g<MVLT_NT_GEMM>((bf16x8*)((bf16*)p.C + idx[sl][it]), a);
      }
    }
  }
}

// ---------------- plan -> launch helpers
// What to launch is decided in gemm_plan.h; a family's launch function maps a plan's template arguments to the instantiation, nothing else.  Every instantiation of
// the GEMM kernels is one entry of the family files' case lists (tests/test_gemm_plan_cpu.py reads them); a plan none of them matches is an error, never another kernel.
static_assert(mvlt_plan::BM == BM && mvlt_plan::NTHREADS == NTHREADS && mvlt_plan::ROW_BYTES == ROW_BYTES && mvlt_plan::TBK == TBK &&
              mvlt_plan::TN_ROWB_BF16 == TElem<bf16>::ROWB && mvlt_plan::TN_ROWB_F32 == TElem<float>::ROWB && mvlt_plan::TN_TILE64_BYTES == DmaTile<64>::BYTES,
              "gemm_plan.h sizes the launches with its own copies of the kernels' constants");
constexpr long tkey(int family, int a, int b = 0, int c = 0, int d = 0, int e = 0, int f = 0) { return ((((((long)family * 400 + a) * 400 + b) * 400 + c) * 400 + d) * 2 + e) * 2 + f; }
// RAISE: the instantiation needs more than the default 64 KB of dynamic LDS
#define MVLT_CASE(RAISE, KERNEL, KEY, ...)                                   \
  case tkey KEY:                                                             \
    if constexpr (RAISE) mvlt_max_lds<KERNEL>();                             \
    MVLT_LAUNCH(KERNEL, grid, block, lds, s, __VA_ARGS__);                   \
    return mvlt_check_launch(who);
#define MVLT_PLAN_LAUNCH_HEAD                                                                                          \
  const dim3 grid((unsigned)p.grid[0], (unsigned)p.grid[1], (unsigned)p.grid[2]), block((unsigned)p.block);            \
  const size_t lds = (size_t)p.lds;                                                                                    \
  const long key = tkey(p.family, p.tp[0], p.tp[1], p.tp[2], p.tp[3], p.tp[4], p.tp[5])
int no_instantiation(const char* who, const mvlt_gemm_plan& p) {
  char name[128] = "?";
  plan_kernel_name(p, name, sizeof(name));
  mvlt_set_error("%s: the plan names %s (family %d), which this library does not instantiate", who, name, p.family);
  return MVLT_ERR_UNSUPPORTED;
}

}  // namespace

// What more than one fused-MLP translation unit uses (mlp.hip and one mlp_<family>.hip per kernel family; the overview is at the top of mlp.hip).
// First part, plain C++ (mlp_plan.h includes it under a host compiler alone): the geometry both the plan and the kernels are built on -- above all the dynamic LDS bytes
// of every instantiation as constexpr functions of its template arguments and the hidden size; each kernel static_asserts its own carve-up of `smem` against them.
// Second part (HIP only): the swizzled tile layout, the operand loader and the epilogue of the two forward / input-gradient kernels, and the per-family launch functions
// mlp.hip calls across the files.
#pragma once
#include <stddef.h>

namespace mvlt_mlp {

constexpr int NT = 256;                         // threads of the 4-wave kernels
constexpr int BM = 128;                         // token rows per workgroup of the forward / input-gradient kernels
constexpr int chunk_units(int C) { return C == 64 ? 64 : 32; }       // hidden units per chunk of mlp_fused_kernel: C * JC = 4096 MACs per token either way
constexpr int wgrad2_waves(int C) { return C == 64 ? 4 : 8; }        // mlp_wgrad2_kernel: one 16-channel tile of dy per wave (the four-wave form needs 446 registers at C = 128)
constexpr int GELU_LUT_BYTES = 13 * 1024;       // the activation table of gelu_lut.inc in LDS: whole 1 KB LDS-DMA instructions (mlp_wgrad.hip asserts it against the table)

// ---- dynamic LDS bytes.  mode 0: forward, 1: input gradient (one more producer-side weight tile, W2^T)
constexpr size_t smax(size_t a, size_t b) { return a > b ? a : b; }
constexpr size_t stage_bytes(int C) { return (size_t)4 * 16 * (C + 4) * 4; }          // mlp_epilogue stages 4 waves x 16 rows x (C + 4) floats over the dead operand tiles
constexpr size_t bias_bytes(int hid) { return (size_t)hid * sizeof(float); }          // fc1's bias behind the weight tiles: the one part that depends on the hidden size
constexpr size_t fused_tiles_bytes(int C, int mode) {                                  // [2][JC][C] W1 chunk | [2][C][JC] Wb chunk | mode 1: [2][JC][C] W2^T chunk
  return (size_t)(2 * chunk_units(C) * C * (mode == 1 ? 2 : 1) + 2 * C * chunk_units(C)) * 2;
}
constexpr size_t fused_lds(int C, int mode, int hid) { return smax(fused_tiles_bytes(C, mode) + bias_bytes(hid), stage_bytes(C)); }
constexpr size_t pipe_tiles_bytes(int C, int mode) {                                   // producer ring [2][1 or 2][32 rows][2 C bytes] | consumer ring [2][C][32 units]
  return (size_t)2 * (mode == 1 ? 2 : 1) * 32 * 2 * C + (size_t)2 * C * 64;
}
constexpr size_t pipe_lds(int C, int mode, int hid) { return smax(pipe_tiles_bytes(C, mode) + bias_bytes(hid), stage_bytes(C)); }
constexpr size_t wgrad_lds(int C) { return (size_t)2 * 128 * C * 2 + (size_t)2 * 2 * 64 * 2 * C; }      // W1, W2^T rows [128][C] each | ring [2][x tile | dy tile] of [64][C]
constexpr size_t wgrad2_flush_bytes(int C, int nw) {                                   // per wave 16 rows of the wider of [C + 8] and [16 JT + 8] bf16: the partial tiles' way out
  return (size_t)nw * 16 * (C + 8 > 16 * (8 / nw) + 8 ? C + 8 : 16 * (8 / nw) + 8) * 2;
}
constexpr size_t wgrad2_lds(int C, int nw) { return smax(wgrad_lds(C) + GELU_LUT_BYTES, wgrad2_flush_bytes(C, nw)); }   // ... | activation table
static_assert(wgrad_lds(64) <= 80 * 1024 && wgrad2_lds(64, 4) <= 80 * 1024 && wgrad_lds(128) <= 160 * 1024 && wgrad2_lds(128, 8) <= 160 * 1024,
              "two workgroups per CU at C = 64, one at C = 128: what the split count of mlp_plan.h fills the chip with");

}  // namespace mvlt_mlp

#ifdef __HIPCC__
#include "common.h"
#include <type_traits>
#include "mlp_plan.h"
#include "../../include/mvlt_hip.h"

// One launch function per family file: the plan's template arguments -> that file's instantiation (a case list, no shape condition), or MVLT_ERR_UNSUPPORTED.
// `who` names the entry point in a launch error.
int mvlt_launch_mlp_fused(const mvlt_mlp_args& a, const mvlt_mlp_plan& p, hipStream_t s, const char* who);     // mlp_fused.hip
int mvlt_launch_mlp_pipe(const mvlt_mlp_args& a, const mvlt_mlp_plan& p, hipStream_t s, const char* who);      // mlp_pipe.hip
int mvlt_launch_mlp_wgrad(const mvlt_mlp_args& a, const mvlt_mlp_plan& p, hipStream_t s, const char* who);     // mlp_wgrad.hip (both weight-gradient families)

namespace {

using mvlt_mlp::NT;

// ---- plan -> launch: a case of a family's list is one instantiation; the launch function checks the launch behind its switch
constexpr int mkey(int a, int b = 0) { return a * 16 + b; }
#define MVLT_MLP_CASE(KERNEL, KEY, ...)                                                                           \
  case mkey KEY:                                                                                                  \
    mvlt_max_lds<KERNEL>();                                                                                       \
    MVLT_LAUNCH(KERNEL, dim3((unsigned)p.grid), dim3((unsigned)p.block), (size_t)p.lds, s, a, ##__VA_ARGS__);     \
    break;
inline int mlp_no_instantiation(const char* who, const mvlt_mlp_plan& p) {
  char name[64] = "?";
  plan_mlp_name(p, name, sizeof(name));
  mvlt_set_error("%s: the plan names %s (family %d), which this library does not instantiate", who, name, p.family);
  return MVLT_ERR_UNSUPPORTED;
}

template <int C> struct MlpGeo { static constexpr int JC = mvlt_mlp::chunk_units(C); };   // hidden units per chunk of mlp_fused_kernel

// element offset inside a [rows][K] bf16 tile with 16-B chunks XOR-swizzled by row (conflict-free fragment reads)
template <int K> __device__ __forceinline__ int toff(int row, int k) {
  constexpr int NCH = K / 8;                 // 16-B chunks per row: 4 (K=32), 8 (K=64) or 16 (K=128)
  int ch = k >> 3;
  int sw = (NCH == 4) ? (ch ^ ((row >> 2) & 3)) : (NCH == 8) ? (ch ^ ((row >> 1) & 7)) : (ch ^ (row & 15));
  return row * K + sw * 8 + (k & 7);
}

__device__ __forceinline__ bf16x8 ldfrag(const bf16* tile_base_elem) { return *(const bf16x8*)tile_base_elem; }

// ---- B-operand fragments of a wave's 32 token rows (x, and dy for the backward): 8 consecutive channels of token fr per lane, straight
// from global memory (used by every hidden chunk, never re-read: no LDS copy); forward: optionally with Block.norm2 folded in
template <int C, int MODE>
__device__ __forceinline__ void mlp_load_rows(const mvlt_mlp_args& p, int m0, int wave, int fr, int fg, bf16x8 (&xfr)[2][C / 32],
                                              bf16x8 (&yfr)[MODE == 1 ? 2 : 1][C / 32]) {
  constexpr int MT = 2, WR = 32, KS_C = C / 32;
  const bf16* X = (const bf16*)p.x;
  const bf16* DY = (const bf16*)p.dy;
  if (MODE == 0 && p.ln_x) {
    // LayerNorm folded into the operand load (Block.norm2): the four fg-lanes of a token hold its whole fp32 row (KS_C x 8 channels
    // each), so the row statistics are two xor-shuffles away; the normalised row is this wave's fc1 operand AND is stored for the
    // backward passes, which replaces a separate LayerNorm launch (fp32 row read + bf16 row written once more)
    const float inv_c = 1.0f / (float)C;
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) {
      const int m = m0 + wave * WR + mt * 16 + fr;
      const bool ok = m < p.M;
      float v[KS_C][8];
      float sum = 0.f;
#pragma unroll
      for (int ks = 0; ks < KS_C; ++ks) {
        f32x4 a = {0.f, 0.f, 0.f, 0.f}, b = {0.f, 0.f, 0.f, 0.f};
        if (ok) {
          const float* src = p.ln_x + (long)m * C + ks * 32 + fg * 8;
          a = *(const f32x4*)src; b = *(const f32x4*)(src + 4);
        }
#pragma unroll
        for (int e = 0; e < 4; ++e) { v[ks][e] = a[e]; v[ks][4 + e] = b[e]; sum += a[e] + b[e]; }
      }
      sum += __shfl_xor(sum, 16); sum += __shfl_xor(sum, 32);
      const float mean = sum * inv_c;
      float q = 0.f;
#pragma unroll
      for (int ks = 0; ks < KS_C; ++ks)
#pragma unroll
        for (int e = 0; e < 8; ++e) { const float d = v[ks][e] - mean; q += d * d; }
      q += __shfl_xor(q, 16); q += __shfl_xor(q, 32);
      const float rstd = rsqrtf(q * inv_c + p.ln_eps);
      if (ok && fg == 0) { p.ln_mean[m] = mean; p.ln_rstd[m] = rstd; }
#pragma unroll
      for (int ks = 0; ks < KS_C; ++ks) {
        const float* gp = p.ln_gamma + ks * 32 + fg * 8;
        const float* bp = p.ln_beta + ks * 32 + fg * 8;
        const f32x4 g0 = *(const f32x4*)gp, g1 = *(const f32x4*)(gp + 4), be0 = *(const f32x4*)bp, be1 = *(const f32x4*)(bp + 4);
        bf16x8 o;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          o[e] = (bf16)((v[ks][e] - mean) * rstd * g0[e] + be0[e]);
          o[4 + e] = (bf16)((v[ks][4 + e] - mean) * rstd * g1[e] + be1[e]);
        }
        if (!ok) o = bf16x8{0, 0, 0, 0, 0, 0, 0, 0};
        xfr[mt][ks] = o;
        if (ok) st_g<MVLT_NT_MLP>((bf16x8*)((bf16*)p.ln_y + (long)m * C + ks * 32 + fg * 8), o);
      }
    }
  } else {
#pragma unroll
  for (int mt = 0; mt < MT; ++mt)
#pragma unroll
    for (int ks = 0; ks < KS_C; ++ks) {
      const int m = m0 + wave * WR + mt * 16 + fr;
      u32x4 v = {0u, 0u, 0u, 0u}, w = {0u, 0u, 0u, 0u};
      if (m < p.M) {
        v = *(const u32x4*)(X + (long)m * C + ks * 32 + fg * 8);
        if (MODE == 1) w = *(const u32x4*)(DY + (long)m * C + ks * 32 + fg * 8);
      }
      xfr[mt][ks] = __builtin_bit_cast(bf16x8, v);
      if (MODE == 1) yfr[mt][ks] = __builtin_bit_cast(bf16x8, w);
    }
  }
}

// ---- epilogue shared by the fused kernels: oacc[i][j][r] = out[token wave*32 + 16 i + 4 fg + r][c = 16 j + fr]
template <int C, int MODE, bool PFALL = true>
__device__ __forceinline__ void mlp_epilogue(const mvlt_mlp_args& p, char* smem, int m0, int tid, f32x4 (&oacc)[2][C / 16]) {
  constexpr int MT = 2, WR = 32, CT = C / 16;
  const int lane = tid & 63, wave = tid >> 6;
  const int fr = lane & 15, fg = lane >> 4;
  // staged per wave through LDS (the operand tiles are dead) so that global traffic is 16-byte, row-contiguous
  // (one 16-token tile at a time: 4 waves x 16 rows x (C+4) floats)
  constexpr int LDW = C + 4, CPR = C / 8, RPI = 64 / CPR;
  float* stage = (float*)smem + wave * 16 * LDW;
  const int ch = lane % CPR;
  const int nc = ch * 8;
  float b2v[8];
#pragma unroll
  for (int e = 0; e < 8; ++e) b2v[e] = (MODE == 0) ? p.b2[nc + e] : 0.f;
  // MODE 1 with lnb_x: the backward of the LayerNorm in front of this MLP (Block.norm2) rides on the epilogue -- the row of
  // d(LN output) is in registers here (CPR lanes x 8 channels), so its two row reductions are log2(CPR) xor-shuffles
  const bool lnb = MODE == 1 && p.lnb_x != nullptr;
  float lgam[8], accg[8], accb[8];
#pragma unroll
  for (int e = 0; e < 8; ++e) { lgam[e] = lnb ? p.lnb_gamma[nc + e] : 0.f; accg[e] = 0.f; accb[e] = 0.f; }
  // Everything the row passes below read from HBM -- the fp32 residual rows (forward), or the LayerNorm input rows, their statistics and
  // the gradient stream's current rows (backward with lnb_x) -- is requested HERE for all of the wave's 32 rows, before the first staging
  // pass: read inside the passes, each of the 2 x NIT row groups paid its own HBM round trip behind the previous group's stores (the
  // epilogue was 52 of 280 us of the stage-1 forward and ~120 of 530 us of the stage-1 input-gradient launch, by ablation)
  constexpr int NIT = 16 / RPI;
  f32x4 pre_a[MT][NIT][2];       // forward: residual row chunk; backward: LayerNorm input row chunk
  u32x4 pre_o[MT][NIT];          // backward: current gradient-stream row chunk (bf16 x 8)
  float pre_mean[MT][NIT], pre_rstd[MT][NIT], pre_rs[MT][NIT], pre_sc[MT][NIT];
  // PFALL = false (three waves per SIMD: the other waves cover the round trip) requests one 16-row tile at a time: half the registers
  auto prefetch = [&](int i) {
#pragma unroll
    for (int it = 0; it < NIT; ++it) {
      const int m = m0 + wave * WR + i * 16 + it * RPI + lane / CPR;
      const bool ok = m < p.M;
      const long idx = (long)(ok ? m : 0) * C + nc;
      const float* src = (MODE == 0) ? (const float*)p.residual + idx : p.lnb_x + idx;
      pre_a[i][it][0] = ld_g<MVLT_NT_LD && MVLT_NT_MLP>((const f32x4*)src);
      pre_a[i][it][1] = ld_g<MVLT_NT_LD && MVLT_NT_MLP>((const f32x4*)(src + 4));
      pre_rs[i][it] = p.row_scale ? p.row_scale[(ok ? m : 0) / p.rows_per_scale] : 1.0f;
      if (MODE == 1) {
        pre_o[i][it] = ld_g<MVLT_NT_LD && MVLT_NT_MLP>((const u32x4*)((const bf16*)p.lnb_dx + idx));
        pre_mean[i][it] = p.lnb_mean[ok ? m : 0];
        pre_rstd[i][it] = p.lnb_rstd[ok ? m : 0];
        pre_sc[i][it] = p.lnb_dx2 ? p.lnb_dx2_scale[(ok ? m : 0) / p.lnb_dx2_rows_per_scale] : 0.f;
      }
    }
  };
  if (PFALL && (MODE == 0 || lnb)) {
#pragma unroll
    for (int i = 0; i < MT; ++i) prefetch(i);
  }
#pragma unroll
  for (int i = 0; i < MT; ++i) {
    if (!PFALL && (MODE == 0 || lnb)) prefetch(i);
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();               // previous tile's reads are done before it is overwritten
#pragma unroll
    for (int j = 0; j < CT; ++j)
#pragma unroll
      for (int r = 0; r < 4; ++r) stage[(4 * fg + r) * LDW + j * 16 + fr] = oacc[i][j][r];
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
#pragma unroll
    for (int it = 0; it < 16 / RPI; ++it) {
      const int rl = it * RPI + lane / CPR;
      const int m = m0 + wave * WR + i * 16 + rl;
      if (m >= p.M) continue;
      f32x4 v0 = *(const f32x4*)(stage + rl * LDW + ch * 8), v1 = *(const f32x4*)(stage + rl * LDW + ch * 8 + 4);
      float v[8] = {v0[0], v0[1], v0[2], v0[3], v1[0], v1[1], v1[2], v1[3]};
      const float rs = (MODE == 0 || lnb) ? pre_rs[i][it] : (p.row_scale ? p.row_scale[m / p.rows_per_scale] : 1.0f);
      const long idx = (long)m * C + nc;
      if (MODE == 0) {
        const f32x4 r0 = pre_a[i][it][0], r1 = pre_a[i][it][1];
        float rr[8] = {r0[0], r0[1], r0[2], r0[3], r1[0], r1[1], r1[2], r1[3]};
#pragma unroll
        for (int e = 0; e < 8; ++e) v[e] = (v[e] + b2v[e]) * rs + rr[e];
        if (p.out) {
          float* O = (float*)p.out + idx;
          st_g<MVLT_NT_MLP>((f32x4*)O, f32x4{v[0], v[1], v[2], v[3]});
          st_g<MVLT_NT_MLP>((f32x4*)(O + 4), f32x4{v[4], v[5], v[6], v[7]});
        }
        if (p.out_op) {                  // MFMA-operand copy of the block output (the last block of a stage writes only this one)
          bf16x8 o;
#pragma unroll
          for (int e = 0; e < 8; ++e) o[e] = (bf16)v[e];
          st_g<MVLT_NT_MLP>((bf16x8*)((bf16*)p.out_op + idx), o);
        }
        if (p.post_y) {
          // LayerNorm of the OUTPUT row (the next block's norm1, reference libs/pvlt.py:141) while the row is here: its CPR lanes hold
          // 8 channels each, so the two-pass statistics are log2(CPR) xor-shuffles; saves that block's LayerNorm launch (fp32 row read)
          float sum = 0.f;
#pragma unroll
          for (int e = 0; e < 8; ++e) sum += v[e];
#pragma unroll
          for (int o = 1; o < CPR; o <<= 1) sum += __shfl_xor(sum, o);
          const float mean = sum * (1.0f / (float)C);
          float q = 0.f;
#pragma unroll
          for (int e = 0; e < 8; ++e) { const float d = v[e] - mean; q += d * d; }
#pragma unroll
          for (int o = 1; o < CPR; o <<= 1) q += __shfl_xor(q, o);
          const float rstd = rsqrtf(q * (1.0f / (float)C) + p.post_eps);
          if (ch == 0) { p.post_mean[m] = mean; p.post_rstd[m] = rstd; }
          const f32x4 g0 = *(const f32x4*)(p.post_gamma + nc), g1 = *(const f32x4*)(p.post_gamma + nc + 4);
          const f32x4 be0 = *(const f32x4*)(p.post_beta + nc), be1 = *(const f32x4*)(p.post_beta + nc + 4);
          bf16x8 o;
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            o[e] = (bf16)((v[e] - mean) * rstd * g0[e] + be0[e]);
            o[4 + e] = (bf16)((v[4 + e] - mean) * rstd * g1[e] + be1[e]);
          }
          st_g<MVLT_NT_MLP>((bf16x8*)((bf16*)p.post_y + idx), o);
        }
      } else if (!lnb) {
        bf16x8 o;
#pragma unroll
        for (int e = 0; e < 8; ++e) o[e] = (bf16)(v[e] * rs);
        st_g<MVLT_NT_MLP>((bf16x8*)((bf16*)p.out + idx), o);
      } else {
        // dx (+)= LayerNorm backward of d(LN output) = v * rs; optional second output dx2 = dx * DropPath factor of the other branch
        const f32x4 x0 = pre_a[i][it][0], x1 = pre_a[i][it][1];
        const bf16x8 old = __builtin_bit_cast(bf16x8, pre_o[i][it]);
        const float xs[8] = {x0[0], x0[1], x0[2], x0[3], x1[0], x1[1], x1[2], x1[3]};
        const float mean = pre_mean[i][it], rstd = pre_rstd[i][it];
        float g[8], xh[8];
        float s1 = 0.f, s2 = 0.f;
#pragma unroll
        for (int e = 0; e < 8; ++e) {
          const float dyn = v[e] * rs;
          xh[e] = (xs[e] - mean) * rstd;
          g[e] = dyn * lgam[e];
          s1 += g[e]; s2 += g[e] * xh[e];
          accg[e] += dyn * xh[e]; accb[e] += dyn;
        }
#pragma unroll
        for (int o = 1; o < CPR; o <<= 1) { s1 += __shfl_xor(s1, o); s2 += __shfl_xor(s2, o); }
        s1 *= 1.0f / (float)C; s2 *= 1.0f / (float)C;
        float dxv[8];
        bf16x8 o1;
#pragma unroll
        for (int e = 0; e < 8; ++e) { dxv[e] = rstd * (g[e] - s1 - xh[e] * s2) + (float)old[e]; o1[e] = (bf16)dxv[e]; }
        st_g<MVLT_NT_MLP>((bf16x8*)((bf16*)p.lnb_dx + idx), o1);
        if (p.lnb_dx2) {
          const float sc = pre_sc[i][it];
          bf16x8 o2;
#pragma unroll
          for (int e = 0; e < 8; ++e) o2[e] = (bf16)(dxv[e] * sc);
          st_g<MVLT_NT_MLP>((bf16x8*)((bf16*)p.lnb_dx2 + idx), o2);
        }
      }
    }
  }
  if (MODE == 1 && lnb) {
    // column sums of this workgroup's rows (d gamma | d beta): lanes with the same channel chunk, then the four waves through LDS,
    // stored plainly per workgroup; mvlt_add_column_sums adds them to the gradient (no same-address atomics from 8000 workgroups)
#pragma unroll
    for (int o = CPR; o < 64; o <<= 1)
#pragma unroll
      for (int e = 0; e < 8; ++e) { accg[e] += __shfl_xor(accg[e], o); accb[e] += __shfl_xor(accb[e], o); }
    __syncthreads();                                  // every wave is done with its staging rows
    float* part = (float*)smem;                      // [4 waves][2 C]
    if (lane < CPR) {
#pragma unroll
      for (int e = 0; e < 8; ++e) { part[wave * 2 * C + nc + e] = accg[e]; part[wave * 2 * C + C + nc + e] = accb[e]; }
    }
    __syncthreads();
    for (int c = tid; c < 2 * C; c += NT)
      p.lnb_partials[(long)blockIdx.x * 2 * C + c] = part[c] + part[2 * C + c] + part[4 * C + c] + part[6 * C + c];
  }
}

}  // namespace
#endif

// Fused MLP of stages 1-2, round-2 forward / input gradient: mlp_fused_kernel and its launch.  Overview: mlp.hip; dispatch: mlp_plan.h.
#include "mlp_common.h"

namespace {

template <int C, int MODE>
__global__ __launch_bounds__(NT) void mlp_fused_kernel(mvlt_mlp_args p) {
  constexpr int JC = MlpGeo<C>::JC;
  constexpr int BM = 128;                    // token rows per workgroup
  constexpr int WR = BM / 4;                 // token rows per wave: each wave is self-contained (producer AND consumer of its rows)
  constexpr int MT = WR / 16;                // 16-token tiles per wave
  constexpr int CT = C / 16;                 // 16-col output tiles (all of C)
  constexpr int KS_C = C / 32;               // k32 steps over C
  extern __shared__ __attribute__((aligned(16))) char smem[];
  bf16* sWa = (bf16*)smem;                                   // [2][JC][C]   W1 chunk
  bf16* sWb = sWa + 2 * JC * C;                              // [2][C][JC]   W2[:, chunk] (mode 0) / W1^T[:, chunk] (mode 1)
  bf16* sWc = sWb + 2 * C * JC;                              // [2][JC][C]   W2^T chunk   (mode 1 only)
  float* sB1 = (float*)(sWc + (MODE == 1 ? 2 * JC * C : 0)); // [hid]        fc1 bias: a global load inside the chunk loop would
                                                             //              wait (vmcnt is in-order) for the weight prefetch too
  static_assert((2 * JC * C + 2 * C * JC + (MODE == 1 ? 2 * JC * C : 0)) * sizeof(bf16) == mvlt_mlp::fused_tiles_bytes(C, MODE) && sizeof(*sB1) * 64 == mvlt_mlp::bias_bytes(64) &&
                BM == mvlt_mlp::BM, "the plan sizes this launch with mlp_common.h's formula: the tiles, then bias_bytes(hid)");
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int fr = lane & 15, fg = lane >> 4;
  const int m0 = blockIdx.x * BM;
  const bf16* X = (const bf16*)p.x;
  const bf16* DY = (const bf16*)p.dy;
  const bf16* Wa = (const bf16*)p.w1;        // [hid][C]
  const bf16* Wb = (const bf16*)p.wb;        // [C][hid]
  const bf16* Wc = (const bf16*)p.wc;        // [hid][C]
  const int hid = p.hid;

  for (int u = tid; u < p.hid; u += NT) sB1[u] = p.b1[u];
  // ---- B-operand fragments of this wave's tokens (x, and dy for the backward): 8 consecutive channels of token fr per
  // lane, straight from global memory (used by every hidden chunk, never re-read: no LDS copy)
  bf16x8 xfr[MT][KS_C], yfr[MODE == 1 ? MT : 1][KS_C];
  mlp_load_rows<C, MODE>(p, m0, wave, fr, fg, xfr, yfr);
  // ---- weight-chunk staging (global -> registers -> LDS), double buffered
  constexpr int WA_IT = JC * (C / 8) / NT;   // 2 (C=64) / 4 (C=128)
  constexpr int WB_IT = C * (JC / 8) / NT;   // 2 / 4
  u32x4 ra[WA_IT], rb[WB_IT], rc[MODE == 1 ? WA_IT : 1];
  auto wload = [&](int jc) {
#pragma unroll
    for (int it = 0; it < WA_IT; ++it) {
      int u = tid + it * NT, r = u / (C / 8), ch = u % (C / 8);
      ra[it] = *(const u32x4*)(Wa + (long)(jc * JC + r) * C + ch * 8);
      if (MODE == 1) rc[it] = *(const u32x4*)(Wc + (long)(jc * JC + r) * C + ch * 8);
    }
#pragma unroll
    for (int it = 0; it < WB_IT; ++it) {
      int u = tid + it * NT, r = u / (JC / 8), ch = u % (JC / 8);
      rb[it] = *(const u32x4*)(Wb + (long)r * hid + jc * JC + ch * 8);
    }
  };
  auto wstore = [&](int buf) {
#pragma unroll
    for (int it = 0; it < WA_IT; ++it) {
      int u = tid + it * NT, r = u / (C / 8), ch = u % (C / 8);
      *(u32x4*)(sWa + buf * JC * C + toff<C>(r, ch * 8)) = ra[it];
      if (MODE == 1) *(u32x4*)(sWc + buf * JC * C + toff<C>(r, ch * 8)) = rc[it];
    }
#pragma unroll
    for (int it = 0; it < WB_IT; ++it) {
      int u = tid + it * NT, r = u / (JC / 8), ch = u % (JC / 8);
      *(u32x4*)(sWb + buf * C * JC + toff<JC>(r, ch * 8)) = rb[it];
    }
  };
  wload(0);
  wstore(0);
  __syncthreads();

  f32x4 oacc[MT][CT];
#pragma unroll
  for (int i = 0; i < MT; ++i)
#pragma unroll
    for (int j = 0; j < CT; ++j) oacc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

  const int nchunks = hid / JC;
  for (int jc = 0; jc < nchunks; ++jc) {
    const int buf = jc & 1;
    if (jc + 1 < nchunks) wload(jc + 1);
    // ---- producers, transposed: tile (jt, mt): rows = hidden units 16 jt.. of the chunk, cols = this wave's tokens 16 mt..
    // A lane ends up with hidden units 16 jt + 4 fg + r of token fr.  Two hidden tiles (jt = 2 pair, 2 pair + 1) give it 8
    // values of one token = one A-operand fragment of the consumer MFMA, with k-slot (fg, jj) <-> hidden unit
    // 32 pair + 16 (jj >> 2) + 4 fg + (jj & 3); the consumer's B operand is read from the W chunk in the same order
    // (two 8-byte LDS reads), so the activation goes from accumulator to operand without touching LDS.
    const bf16* wa = sWa + buf * JC * C;
    const bf16* wc = sWc + buf * JC * C;
    bf16x8 gfrag[JC / 32][MT];
#pragma unroll
    for (int jt = 0; jt < JC / 16; ++jt) {
      const int jrow = jt * 16 + fr;                   // A-operand row (hidden unit inside the chunk)
      bf16x8 af[KS_C], cf[MODE == 1 ? KS_C : 1];
#pragma unroll
      for (int ks = 0; ks < KS_C; ++ks) {
        af[ks] = ldfrag(wa + toff<C>(jrow, ks * 32 + fg * 8));
        if (MODE == 1) cf[ks] = ldfrag(wc + toff<C>(jrow, ks * 32 + fg * 8));
      }
      const int jl = jt * 16 + 4 * fg;                 // the four hidden units this lane ends up with: jl + r
      f32x4 b1v = *(const f32x4*)(sB1 + jc * JC + jl);
#pragma unroll
      for (int mt = 0; mt < MT; ++mt) {
        const int mrow = wave * WR + mt * 16 + fr;     // token (column fr of the tile)
        f32x4 h = {0.f, 0.f, 0.f, 0.f}, dg = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int ks = 0; ks < KS_C; ++ks) {
          h = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af[ks], xfr[mt][ks], h, 0, 0, 0);
          if (MODE == 1) dg = __builtin_amdgcn_mfma_f32_16x16x32_bf16(cf[ks], yfr[mt][ks], dg, 0, 0, 0);
        }
#pragma unroll
        for (int r = 0; r < 4; r += 2) {
          const f32x2 hv = f32x2{h[r], h[r + 1]} + f32x2{b1v[r], b1v[r + 1]};
          // (the polynomial forms, not the activation table of mlp_wgrad.hip: four waves per SIMD already hide them and the gather's LDS latency is not hidden --
          //  by table the input gradient went 301 -> 306 us at C = 128, the forward 265 -> 283 / 204 -> 210 us)
          const f32x2 gv = (MODE == 0) ? gelu_fast2(hv) : f32x2{dg[r], dg[r + 1]} * gelu_fast_grad2(hv);
          gfrag[jt >> 1][mt][(jt & 1) * 4 + r] = (bf16)gv[0];
          gfrag[jt >> 1][mt][(jt & 1) * 4 + r + 1] = (bf16)gv[1];
          h[r] = hv[0]; h[r + 1] = hv[1];
        }
        if (MODE == 0 && p.h_out && m0 + mrow < p.M) {
          bf16x4 h4 = {(bf16)h[0], (bf16)h[1], (bf16)h[2], (bf16)h[3]};
          *(bf16x4*)((bf16*)p.h_out + (long)(m0 + mrow) * hid + jc * JC + jl) = h4;
        }
      }
    }
    // ---- consumer: out[this wave's tokens][C] += G[tokens][64] . Wb[C][64]^T
    const bf16* wb = sWb + buf * C * JC;
#pragma unroll
    for (int pair = 0; pair < JC / 32; ++pair) {
#pragma unroll
      for (int j = 0; j < CT; ++j) {
        const bf16x4 b0 = *(const bf16x4*)(wb + toff<JC>(j * 16 + fr, pair * 32 + 4 * fg));
        const bf16x4 b1 = *(const bf16x4*)(wb + toff<JC>(j * 16 + fr, pair * 32 + 16 + 4 * fg));
        const bf16x8 bfr = {b0[0], b0[1], b0[2], b0[3], b1[0], b1[1], b1[2], b1[3]};
#pragma unroll
        for (int i = 0; i < MT; ++i) oacc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(gfrag[pair][i], bfr, oacc[i][j], 0, 0, 0);
      }
    }
    if (jc + 1 < nchunks) wstore(buf ^ 1);
    __syncthreads();                                   // weight double buffer: next chunk visible, this one free next time
  }

  mlp_epilogue<C, MODE>(p, smem, m0, tid, oacc);
}

}  // namespace

// ------------------------------------------------------------------------------------------------ plan -> launch
#define FUSED(C, MODE) MVLT_MLP_CASE((mlp_fused_kernel<C, MODE>), (C, MODE))
int mvlt_launch_mlp_fused(const mvlt_mlp_args& a, const mvlt_mlp_plan& p, hipStream_t s, const char* who) {
  switch (mkey(p.tp[0], p.tp[1])) {
    FUSED(64, 0) FUSED(64, 1) FUSED(128, 0) FUSED(128, 1)
    default: return mlp_no_instantiation(who, p);
  }
  return mvlt_check_launch(who);
}

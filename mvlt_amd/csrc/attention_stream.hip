// SR-attention, key-streamed forward and backward (any number of keys): both kernels and their launches.  Overview: attention.hip; dispatch: attn_plan.h.
#include "attention_common.h"

namespace {

// ------------------------------------------------------------------------------------------------ streamed forward (any M)
// The LDS-resident kernels above hold all of K and V^T of a (batch, head); past 320 keys (bf16) / 288 keys (fp32) that no longer fits.
// Here the keys stream through a 2-deep LDS ring in blocks of KB keys (K rows swizzled, V^T transposed, the layouts of attn_fwd_kernel):
// block j + 1 is loaded into registers while block j's MFMAs run and written into the other ring slot behind them -- one workgroup
// barrier per block.  Same lane layout as attn_fwd_kernel (S^T = K Q^T: a lane owns one query's scores; P^T is the B operand of
// O^T = V^T P^T) with an online softmax over the blocks: running maximum and sum per query, O rescaled whenever a block raises the
// maximum.  Only the last block can hold padded keys (staged as zeros, masked to -inf).  A workgroup is 4 waves x 32 queries; its
// query chunk reads K / V once (from L2 after the first chunk of the (batch, head) on that XCD).

template <typename T, int KB>
__global__ __launch_bounds__(NT, 2) void attn_fwd_stream_kernel(mvlt_attn_args p, int nq_chunks) {
  constexpr int NKT = KB / 32;                  // key tiles per block
  constexpr int VS = KB + 4;                    // V^T row stride (elements)
  constexpr int PC = Lds<T>::PC, NCH = Lds<T>::NCH;
  constexpr int SLOT = KB * HD + HD * VS;       // elements of one ring slot: K [KB][64] swizzled | V^T [64][VS]
  constexpr int LPT = KB * NCH / NT;            // 16-byte pieces per thread, block and tensor
  static_assert(KB % 32 == 0 && (KB * NCH) % NT == 0, "key block");
  extern __shared__ __attribute__((aligned(16))) char smem[];
  T* ring = (T*)smem;
  static_assert(2 * SLOT * sizeof(T) == mvlt_attn::fwd_stream_lds(sizeof(T), KB), "the plan sizes this launch with attention_common.h's formula");

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int g = lane >> 5, l31 = lane & 31;
  const int bid = blockIdx.x;
  const int xcd = bid & 7, j = bid >> 3;
  const int gidx = xcd + 8 * (j / nq_chunks);
  const int chunk_id = j % nq_chunks;
  if (gidx >= p.B * p.H) return;
  const int b = gidx / p.H, h = gidx % p.H;

  const T* Qg = (const T*)p.Q + (long)b * p.N * p.ldq + h * HD;
  const T* Kg = (const T*)p.KV + (long)b * p.M * p.ldkv + p.k_off + h * HD;
  const T* Vg = (const T*)p.KV + (long)b * p.M * p.ldkv + p.v_off + h * HD;
  T* Og = (T*)p.O + (long)b * p.N * p.ldo + h * HD;
  const int nblk = (p.M + KB - 1) / KB;

  u32x4 kst[LPT], vst[LPT];
  auto fetch = [&](int blk) {                   // block blk's K / V rows -> registers; keys >= M are zero
#pragma unroll
    for (int i = 0; i < LPT; ++i) {
      const int u = tid + i * NT, r = u / NCH, c = u % NCH, key = blk * KB + r;
      kst[i] = u32x4{0u, 0u, 0u, 0u};
      vst[i] = u32x4{0u, 0u, 0u, 0u};
      if (key < p.M) {
        kst[i] = *(const u32x4*)(Kg + (long)key * p.ldkv + c * PC);
        vst[i] = *(const u32x4*)(Vg + (long)key * p.ldkv + c * PC);
      }
    }
  };
  auto put = [&](int slot) {                    // registers -> ring slot: K swizzled, V transposed
    T* sK = ring + slot * SLOT;
    T* sVt = sK + KB * HD;
#pragma unroll
    for (int i = 0; i < LPT; ++i) {
      const int u = tid + i * NT, r = u / NCH, c = u % NCH;
      *(u32x4*)(sK + Lds<T>::off(r, c * PC)) = kst[i];
      T ve[PC];
      *(u32x4*)ve = vst[i];
#pragma unroll
      for (int e = 0; e < PC; ++e) sVt[(c * PC + e) * VS + r] = ve[e];
    }
  };
  fetch(0);
  put(0);

  const float sl2 = p.scale * 1.44269504088896340736f;
  const int q_begin = chunk_id * STREAM_QPW;
  const int q_end = min(p.N, q_begin + STREAM_QPW);
  const int q = q_begin + wave * 32 + l31;
  const bool q_ok = q < q_end;
  Frag<T> qf[4];
#pragma unroll
  for (int s = 0; s < 4; ++s) qf[s] = q_ok ? load_frag8<T>(Qg + (long)q * p.ldq + 16 * s + 8 * g) : zero_frag<T>();
  f32x16 oacc[2];
#pragma unroll
  for (int dt = 0; dt < 2; ++dt)
#pragma unroll
    for (int r = 0; r < 16; ++r) oacc[dt][r] = 0.f;
  float m_run = -INFINITY, sum_loc = 0.f;
  __syncthreads();

  for (int blk = 0; blk < nblk; ++blk) {
    const T* sK = ring + (blk & 1) * SLOT;
    const T* sVt = sK + KB * HD;
    f32x16 acc[NKT];
    Frag<T> kf[2][4];
#pragma unroll
    for (int s = 0; s < 4; ++s) kf[0][s] = load_frag8<T>(sK + Lds<T>::off(l31, 16 * s + 8 * g));
#pragma unroll
    for (int ti = 0; ti < NKT; ++ti) {
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[ti][r] = 0.f;
      if (ti + 1 < NKT) {
#pragma unroll
        for (int s = 0; s < 4; ++s) kf[(ti + 1) & 1][s] = load_frag8<T>(sK + Lds<T>::off((ti + 1) * 32 + l31, 16 * s + 8 * g));
      }
#pragma unroll
      for (int s = 0; s < 4; ++s) mma32(acc[ti], kf[ti & 1][s], qf[s]);            // rows = keys, cols = queries
      __builtin_amdgcn_sched_barrier(0);
    }
    // the next block in flight under this block's softmax and P V (issued here, not earlier: the staging registers and the K
    // fragments of the score loop are not live at the same time)
    if (blk + 1 < nblk) fetch(blk + 1);
    // acc[ti][r] = S[q = l31][key = KB blk + 32 ti + (r&3) + 8 (r>>2) + 4 g]
    const int kvalid = p.M - blk * KB;          // >= 1; < KB only in the last block
    float mb = -INFINITY;
    if (kvalid >= KB) {
#pragma unroll
      for (int ti = 0; ti < NKT; ++ti)
#pragma unroll
        for (int r = 0; r < 16; ++r) mb = fmaxf(mb, acc[ti][r]);
    } else {
#pragma unroll
      for (int ti = 0; ti < NKT; ++ti)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int key = 32 * ti + (r & 3) + 8 * (r >> 2) + 4 * g;
          const float sv = key < kvalid ? acc[ti][r] : -INFINITY;
          acc[ti][r] = sv;
          mb = fmaxf(mb, sv);
        }
    }
    mb = fmaxf(mb, __shfl_xor(mb, 32));
    const float m_new = fmaxf(m_run, mb);       // finite: every block holds >= 1 valid key
    if (blk > 0) {
      const float alpha = exp2f((m_run - m_new) * sl2);
      sum_loc *= alpha;
#pragma unroll
      for (int dt = 0; dt < 2; ++dt)
#pragma unroll
        for (int r = 0; r < 16; ++r) oacc[dt][r] *= alpha;
    }
    m_run = m_new;
    const float mneg = -m_new * sl2;
#pragma unroll
    for (int ti = 0; ti < NKT; ++ti)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        float e;
        if constexpr (sizeof(T) == 2) e = __builtin_amdgcn_exp2f(__builtin_fmaf(acc[ti][r], sl2, mneg));
        else e = exp2f((acc[ti][r] - m_new) * sl2);
        acc[ti][r] = e;
        sum_loc += e;
      }
    Frag<T> vf[2][2];
#pragma unroll
    for (int dt = 0; dt < 2; ++dt) { const T* vr = sVt + (32 * dt + l31) * VS + 4 * g; vf[0][dt] = load_frag44<T>(vr, vr + 8); }
#pragma unroll
    for (int u = 0; u < 2 * NKT; ++u) {
      const int ti = u >> 1, s2 = u & 1;
      if (u + 1 < 2 * NKT) {
        const int kb = 32 * ((u + 1) >> 1) + 16 * ((u + 1) & 1) + 4 * g;
#pragma unroll
        for (int dt = 0; dt < 2; ++dt) { const T* vr = sVt + (32 * dt + l31) * VS + kb; vf[(u + 1) & 1][dt] = load_frag44<T>(vr, vr + 8); }
      }
      Frag<T> pf;                               // B operand: P^T, k-slot (g, jj) <-> key 32 ti + 16 s2 + 4g + 8 (jj>>2) + (jj&3)
#pragma unroll
      for (int jj = 0; jj < 8; ++jj) pf.v[jj] = (T)acc[ti][8 * s2 + jj];
#pragma unroll
      for (int dt = 0; dt < 2; ++dt) mma32(oacc[dt], vf[u & 1][dt], pf);            // rows = d, cols = queries
      __builtin_amdgcn_sched_barrier(0);
    }
    // the other slot was last read in block blk - 1, before the barrier that ended it
    if (blk + 1 < nblk) put((blk + 1) & 1);
    __syncthreads();
  }
  const float sum = sum_loc + __shfl_xor(sum_loc, 32);
  const float inv = 1.0f / sum;
  if (q_ok) {
#pragma unroll
    for (int dt = 0; dt < 2; ++dt)
#pragma unroll
      for (int rq = 0; rq < 4; ++rq) {
        T o4[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) o4[e] = (T)(oacc[dt][4 * rq + e] * inv);
        T* dst = Og + (long)q * p.ldo + 32 * dt + 8 * rq + 4 * g;
        if constexpr (sizeof(T) == 2) *(u32x2*)dst = *(u32x2*)o4; else *(u32x4*)dst = *(u32x4*)o4;
      }
    if (g == 0 && p.lse) p.lse[((long)b * p.H + h) * p.N + q] = m_run * p.scale + logf(sum);
  }
}


// ------------------------------------------------------------------------------------------------ streamed backward (any M)
// Once lse is known the backward splits exactly over key blocks.  One workgroup per (batch, head, chunk of <= 128 queries).  Outer
// loop: blocks of KB = 16 NW TPW keys; K^T staged in LDS and each wave's K / V fragments in registers as attn_bwd_kernel does it for
// all keys.  Inner loop: the chunk's 32-query tiles, each the same S / dP -> P / dS -> dV, dK, dQ step as attn_bwd_kernel with P
// recomputed from lse.  dK / dV of the block accumulate in registers over the tiles and leave at the end of the block (plain stores
// with one chunk -- bf16 or fp32 dKV --, fp32 atomics into the caller-zeroed dKV otherwise); dQ of the chunk accumulates in an fp32
// LDS tile over the blocks (every 16 x 16 piece always owned by the same wave: deterministic) and is stored once at the end.
// D = rowsum(dO * O) and lse of the chunk's queries are computed once, up front, into LDS.

template <typename T, int NW, int TPW>
__global__ __launch_bounds__(NW * 64, 2) void attn_bwd_stream_kernel(mvlt_attn_bwd_args p, int nq_chunks, int q_per_wg) {
  constexpr int NTH = NW * 64;
  constexpr int KB = NW * TPW * 16;             // keys per block
  constexpr int PC = Lds<T>::PC, NCH = Lds<T>::NCH;
  constexpr int PAD = 16 / sizeof(T);
  constexpr int KS = KB + PAD;                  // row stride of sKt and sdS (elements)
  constexpr int QS = 32 + PAD;                  // row stride of sQt / sdOt
  extern __shared__ __attribute__((aligned(16))) char smem[];
  T* sKt = (T*)smem;                            // [64 d][KS]   K^T of the block
  T* sdS = sKt + HD * KS;                       // [32 q][KS]
  T* sQt = sdS + 32 * KS;                       // [64 d][QS]   Q^T tile
  T* sdOt = sQt + HD * QS;                      // [64 d][QS]   dO^T tile
  float* sdQ = (float*)(sdOt + HD * QS);        // [STREAM_QPW][DQS] fp32 dQ of the chunk
  float* sD = sdQ + STREAM_QPW * DQS;           // [STREAM_QPW]
  float* sL = sD + STREAM_QPW;                  // [STREAM_QPW]
  static_assert((HD * KS + 32 * KS + 2 * HD * QS) * sizeof(T) + STREAM_QPW * (DQS + 2) * sizeof(float) == mvlt_attn::bwd_stream_lds(sizeof(T), NW, TPW), "the plan sizes this launch with attention_common.h's formula");

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int fr = lane & 15, fg = lane >> 4;
  const int bid = blockIdx.x;
  const int xcd = bid & 7, jb = bid >> 3;
  const int gidx = xcd + 8 * (jb / nq_chunks);
  const int chunk_id = jb % nq_chunks;
  if (gidx >= p.B * p.H) return;
  const int b = gidx / p.H, h = gidx % p.H;

  const T* Qg = (const T*)p.Q + (long)b * p.N * p.ldq + h * HD;
  const T* Og = (const T*)p.O + (long)b * p.N * p.ldo + h * HD;
  const T* dOg = (const T*)p.dO + (long)b * p.N * p.ldo + h * HD;
  const T* Kg = (const T*)p.KV + (long)b * p.M * p.ldkv + p.k_off + h * HD;
  const T* Vg = (const T*)p.KV + (long)b * p.M * p.ldkv + p.v_off + h * HD;
  T* dQg = (T*)p.dQ + (long)b * p.N * p.ldq + h * HD;
  const float* Lg = p.lse + ((long)b * p.H + h) * p.N;
  const int q_begin = chunk_id * q_per_wg;
  const int q_end = min(p.N, q_begin + q_per_wg);

  // ---- D, lse of the chunk's queries; dQ tile zeroed
  for (int u = tid; u < q_per_wg * NCH; u += NTH) {
    const int r = u / NCH, c = u % NCH, q = q_begin + r;
    u32x4 dov = {0u, 0u, 0u, 0u}, ov = {0u, 0u, 0u, 0u};
    if (q < q_end) {
      dov = *(const u32x4*)(dOg + (long)q * p.ldo + c * PC);
      ov = *(const u32x4*)(Og + (long)q * p.ldo + c * PC);
    }
    T de[PC], oe[PC];
    *(u32x4*)de = dov; *(u32x4*)oe = ov;
    float dsum = 0.f;
#pragma unroll
    for (int e = 0; e < PC; ++e) dsum += (float)de[e] * (float)oe[e];
#pragma unroll
    for (int o = NCH / 2; o > 0; o >>= 1) dsum += __shfl_xor(dsum, o);
    if (c == 0) { sD[r] = dsum; sL[r] = q < q_end ? Lg[q] : 0.f; }
  }
  for (int u = tid; u < q_per_wg * DQS; u += NTH) sdQ[u] = 0.f;

  const float sl2 = p.scale * 1.44269504088896340736f;
  const float l2e = 1.44269504088896340736f;
  const int nblk = (p.M + KB - 1) / KB;
  for (int blk = 0; blk < nblk; ++blk) {
    const int k0 = blk * KB;
    __syncthreads();                                   // every wave is done with the previous block's K^T (dQ step)
    for (int u = tid; u < KB * NCH; u += NTH) {
      const int r = u / NCH, c = u % NCH;
      u32x4 kv = {0u, 0u, 0u, 0u};
      if (k0 + r < p.M) kv = *(const u32x4*)(Kg + (long)(k0 + r) * p.ldkv + c * PC);
      T ke[PC];
      *(u32x4*)ke = kv;
#pragma unroll
      for (int e = 0; e < PC; ++e) sKt[(c * PC + e) * KS + r] = ke[e];
    }
    Frag<T> kreg[TPW][2], vreg[TPW][2];
#pragma unroll
    for (int t = 0; t < TPW; ++t) {
      const int key = k0 + (wave * TPW + t) * 16 + fr;
#pragma unroll
      for (int s = 0; s < 2; ++s) {
        if (key < p.M) {
          kreg[t][s] = load_frag8<T>(Kg + (long)key * p.ldkv + 32 * s + 8 * fg);
          vreg[t][s] = load_frag8<T>(Vg + (long)key * p.ldkv + 32 * s + 8 * fg);
        } else {
          kreg[t][s] = zero_frag<T>();
          vreg[t][s] = zero_frag<T>();
        }
      }
    }
    f32x4 dKacc[TPW][4], dVacc[TPW][4];
#pragma unroll
    for (int t = 0; t < TPW; ++t)
#pragma unroll
      for (int dt = 0; dt < 4; ++dt) { dKacc[t][dt] = f32x4{0.f, 0.f, 0.f, 0.f}; dVacc[t][dt] = f32x4{0.f, 0.f, 0.f, 0.f}; }

    for (int q0 = q_begin; q0 < q_end; q0 += 32) {
      const int lq0 = q0 - q_begin;                    // chunk-local row of the tile
      // ---- (a) Q^T, dO^T tiles
      for (int u = tid; u < 32 * NCH; u += NTH) {
        const int r = u / NCH, c = u % NCH, q = q0 + r;
        u32x4 qv = {0u, 0u, 0u, 0u}, dov = {0u, 0u, 0u, 0u};
        if (q < q_end) {
          qv = *(const u32x4*)(Qg + (long)q * p.ldq + c * PC);
          dov = *(const u32x4*)(dOg + (long)q * p.ldo + c * PC);
        }
        T qe[PC], de[PC];
        *(u32x4*)qe = qv; *(u32x4*)de = dov;
#pragma unroll
        for (int e = 0; e < PC; ++e) {
          sQt[(c * PC + e) * QS + r] = qe[e];
          sdOt[(c * PC + e) * QS + r] = de[e];
        }
      }
      Frag<T> qf[2][2], dof[2][2];
#pragma unroll
      for (int qs = 0; qs < 2; ++qs) {
        const int q = q0 + qs * 16 + fr;
#pragma unroll
        for (int s = 0; s < 2; ++s) {
          if (q < q_end) {
            qf[qs][s] = load_frag8<T>(Qg + (long)q * p.ldq + 32 * s + 8 * fg);
            dof[qs][s] = load_frag8<T>(dOg + (long)q * p.ldo + 32 * s + 8 * fg);
          } else {
            qf[qs][s] = zero_frag<T>();
            dof[qs][s] = zero_frag<T>();
          }
        }
      }
      __syncthreads();                                 // (b) tiles staged (and, on the first tile, K^T, D, lse, the zeroed dQ)

      // ---- (c) per owned key tile: S, dP -> P, dS ; dV += P^T dO ; dK += dS^T Q ; park dS in LDS
#pragma unroll
      for (int t = 0; t < TPW; ++t) {
        const int kl = (wave * TPW + t) * 16 + fr;     // key inside the block
        const bool key_ok = k0 + kl < p.M;
        Frag<T> pfrag, dsfrag;
#pragma unroll
        for (int qs = 0; qs < 2; ++qs) {
          f32x4 sacc = {0.f, 0.f, 0.f, 0.f}, pacc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
          for (int s = 0; s < 2; ++s) {
            mma16(sacc, qf[qs][s], kreg[t][s]);        // S[q = 16 qs + 4 fg + r][key]
            mma16(pacc, dof[qs][s], vreg[t][s]);       // dP
          }
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const int ql = qs * 16 + 4 * fg + r;
            const float pv = key_ok ? exp2f(sacc[r] * sl2 - sL[lq0 + ql] * l2e) : 0.f;
            const float dsv = pv * (pacc[r] - sD[lq0 + ql]) * p.scale;
            pfrag.v[qs * 4 + r] = (T)pv;
            dsfrag.v[qs * 4 + r] = (T)dsv;
            sdS[ql * KS + kl] = (T)dsv;
          }
        }
#pragma unroll
        for (int dt = 0; dt < 4; ++dt) {
          const T* a = sQt + (dt * 16 + fr) * QS + 4 * fg;
          const T* c2 = sdOt + (dt * 16 + fr) * QS + 4 * fg;
          Frag<T> dotf = load_frag44<T>(c2, c2 + 16);
          Frag<T> qtf = load_frag44<T>(a, a + 16);
          mma16(dVacc[t][dt], pfrag, dotf);            // dV[key = tile*16 + 4 fg + r][d = 16 dt + fr]
          mma16(dKacc[t][dt], dsfrag, qtf);
        }
        __builtin_amdgcn_sched_barrier(0);
      }
      __syncthreads();                                 // (d)

      // ---- (e) dQ[32 x 64] += dS[32 x KB] K[KB x 64] of this block: 8 output tiles (16 x 16), tile -> wave fixed
      for (int tile = wave; tile < 8; tile += NW) {
        const int qs = tile >> 2, dt = tile & 3;
        f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int ks = 0; ks < KB / 32; ++ks) {
          Frag<T> a = load_frag8<T>(sdS + (qs * 16 + fr) * KS + 32 * ks + 8 * fg);
          Frag<T> bb = load_frag8<T>(sKt + (dt * 16 + fr) * KS + 32 * ks + 8 * fg);
          mma16(acc, a, bb);
        }
#pragma unroll
        for (int r = 0; r < 4; ++r) sdQ[(lq0 + qs * 16 + 4 * fg + r) * DQS + dt * 16 + fr] += acc[r];
      }
    }
    // ---- flush the block's dK / dV
#pragma unroll
    for (int t = 0; t < TPW; ++t)
#pragma unroll
      for (int dt = 0; dt < 4; ++dt)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int key = k0 + (wave * TPW + t) * 16 + 4 * fg + r;
          if (key < p.M) {
            const long ok = ((long)b * p.M + key) * p.lddkv + p.k_off + h * HD + dt * 16 + fr;
            const long ov = ((long)b * p.M + key) * p.lddkv + p.v_off + h * HD + dt * 16 + fr;
            if (nq_chunks == 1 && p.dkv_dtype == 0) {
              ((bf16*)p.dKV)[ok] = (bf16)dKacc[t][dt][r];
              ((bf16*)p.dKV)[ov] = (bf16)dVacc[t][dt][r];
            } else if (nq_chunks == 1) {
              ((float*)p.dKV)[ok] = dKacc[t][dt][r];
              ((float*)p.dKV)[ov] = dVacc[t][dt][r];
            } else {
              atomicAdd((float*)p.dKV + ok, dKacc[t][dt][r]);
              atomicAdd((float*)p.dKV + ov, dVacc[t][dt][r]);
            }
          }
        }
  }
  __syncthreads();
  // ---- dQ of the chunk, in the operand dtype
  for (int u = tid; u < q_per_wg * NCH; u += NTH) {
    const int r = u / NCH, c = u % NCH, q = q_begin + r;
    if (q >= q_end) continue;
    T out[PC];
#pragma unroll
    for (int e = 0; e < PC; ++e) out[e] = (T)sdQ[r * DQS + c * PC + e];
    *(u32x4*)(dQg + (long)q * p.ldq + c * PC) = *(const u32x4*)out;
  }
}

}  // namespace

// ------------------------------------------------------------------------------------------------ plan -> launch
int mvlt_launch_attn_fwd_stream(const mvlt_attn_args& a, const mvlt_attn_plan& p, hipStream_t s) {
  const char* const who = "mvlt_sr_attention_fwd";
#define FWD_STREAM(T, DT) MVLT_ATTN_CASE((attn_fwd_stream_kernel<T, StreamKB<T>::fwd>), (DT, StreamKB<T>::fwd), p.nq_chunks)
  switch (tkey(p.tp[0], p.tp[1])) {
    FWD_STREAM(bf16, 0) FWD_STREAM(float, 1)
  }
#undef FWD_STREAM
  return attn_no_instantiation(who, p);
}

int mvlt_launch_attn_bwd_stream(const mvlt_attn_bwd_args& a, const mvlt_attn_plan& p, hipStream_t s) {
  const char* const who = "mvlt_sr_attention_bwd";
#define BWD_STREAM(T, DT) \
  MVLT_ATTN_CASE((attn_bwd_stream_kernel<T, mvlt_attn::STREAM_BWD_NW, StreamKB<T>::bwd_tpw>), (DT, mvlt_attn::STREAM_BWD_NW, StreamKB<T>::bwd_tpw), p.nq_chunks, p.q_per_wg)
  switch (tkey(p.tp[0], p.tp[1], p.tp[2])) {
    BWD_STREAM(bf16, 0) BWD_STREAM(float, 1)
  }
#undef BWD_STREAM
  return attn_no_instantiation(who, p);
}

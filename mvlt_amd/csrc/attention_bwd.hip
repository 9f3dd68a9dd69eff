// SR-attention, resident fp32 backward: attn_bwd_kernel and its launch.  Overview: attention.hip; dispatch: attn_plan.h.
#include "attention_common.h"

namespace {

// ------------------------------------------------------------------------------------------------ backward
// dQ = dS K, dK = dS^T Q, dV = P^T dO with P = exp(S*scale - lse), dS = P (dP - D) scale, dP = dO V^T, D = rowsum(dO*O).
// Work split (per (batch, head, query chunk) workgroup): wave w OWNS key tiles [w*TPW, (w+1)*TPW) x 16 keys: its K/V
// fragments stay in registers for the whole kernel and its dK/dV tiles accumulate in registers over all query
// tiles; one fp32 atomic flush at the end.  Per 32-query tile: S and dP via 16x16x32 MFMA (rows = queries), P/dS
// are re-used from the accumulators as the A operand of dV/dK (k-slots = queries), dS is also parked in LDS as
// [q][key] so that dQ (k = all keys) is computed by all waves against the LDS-resident K^T.
template <typename T, int NW, int TPW>
__global__ __launch_bounds__(NW * 64, NW == 4 ? 2 : 1) void attn_bwd_kernel(mvlt_attn_bwd_args p, int nq_chunks, int q_per_wg) {
  constexpr int NTH = NW * 64;
  constexpr int MP = NW * TPW * 16;           // padded keys (multiple of 32)
  constexpr int PC = Lds<T>::PC, NCH = Lds<T>::NCH;
  constexpr int PAD = 16 / sizeof(T);         // 16 B of padding per row
  constexpr int KS = MP + PAD;                // row stride of sKt and sdS (elements)
  constexpr int QS = 32 + PAD;                // row stride of sQt / sdOt
  extern __shared__ __attribute__((aligned(16))) char smem[];
  T* sKt = (T*)smem;                          // [64 d][KS]   K^T
  T* sdS = sKt + HD * KS;                     // [32 q][KS]
  T* sQt = sdS + 32 * KS;                     // [64 d][QS]   Q^T tile
  T* sdOt = sQt + HD * QS;                    // [64 d][QS]   dO^T tile
  float* sD = (float*)(sdOt + HD * QS);       // [32]
  float* sL = sD + 32;                        // [32]
  static_assert((HD * KS + 32 * KS + 2 * HD * QS) * sizeof(T) + 64 * sizeof(float) == mvlt_attn::bwd_lds(sizeof(T), NW, TPW), "the plan sizes this launch with attention_common.h's formula");

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
  float* dKg = (float*)p.dKV + (long)b * p.M * p.lddkv + p.k_off + h * HD;
  float* dVg = (float*)p.dKV + (long)b * p.M * p.lddkv + p.v_off + h * HD;
  const float* Lg = p.lse + ((long)b * p.H + h) * p.N;

  // K^T into LDS (all keys), zero beyond M
  for (int u = tid; u < MP * NCH; u += NTH) {
    int r = u / NCH, c = u % NCH;
    u32x4 kv = {0u, 0u, 0u, 0u};
    if (r < p.M) kv = *(const u32x4*)(Kg + (long)r * p.ldkv + c * PC);
    T ke[PC];
    *(u32x4*)ke = kv;
#pragma unroll
    for (int e = 0; e < PC; ++e) sKt[(c * PC + e) * KS + r] = ke[e];
  }
  // this wave's K / V fragments (B operands: n = key = fr, k = d)
  Frag<T> kreg[TPW][2], vreg[TPW][2];
#pragma unroll
  for (int t = 0; t < TPW; ++t) {
    int key = (wave * TPW + t) * 16 + fr;
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

  const float sl2 = p.scale * 1.44269504088896340736f;
  const float l2e = 1.44269504088896340736f;
  const int q_begin = chunk_id * q_per_wg;
  const int q_end = min(p.N, q_begin + q_per_wg);

  for (int q0 = q_begin; q0 < q_end; q0 += 32) {
    // ---- (a) stage Q^T, dO^T tiles, D and lse for 32 queries
    for (int u = tid; u < 32 * NCH; u += NTH) {
      int r = u / NCH, c = u % NCH;
      int q = q0 + r;
      u32x4 qv = {0u, 0u, 0u, 0u}, dov = {0u, 0u, 0u, 0u}, ov = {0u, 0u, 0u, 0u};
      if (q < q_end) {
        qv = *(const u32x4*)(Qg + (long)q * p.ldq + c * PC);
        dov = *(const u32x4*)(dOg + (long)q * p.ldo + c * PC);
        ov = *(const u32x4*)(Og + (long)q * p.ldo + c * PC);
      }
      T qe[PC], de[PC], oe[PC];
      *(u32x4*)qe = qv; *(u32x4*)de = dov; *(u32x4*)oe = ov;
      float dsum = 0.f;
#pragma unroll
      for (int e = 0; e < PC; ++e) {
        sQt[(c * PC + e) * QS + r] = qe[e];
        sdOt[(c * PC + e) * QS + r] = de[e];
        dsum += (float)de[e] * (float)oe[e];
      }
#pragma unroll
      for (int o = NCH / 2; o > 0; o >>= 1) dsum += __shfl_xor(dsum, o);
      if (c == 0) sD[r] = dsum;
    }
    if (tid < 32) sL[tid] = (q0 + tid < q_end) ? Lg[q0 + tid] : 0.f;
    // A-operand fragments of Q and dO (rows = queries) straight from global
    Frag<T> qf[2][2], dof[2][2];
#pragma unroll
    for (int qs = 0; qs < 2; ++qs) {
      int q = q0 + qs * 16 + fr;
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
    __syncthreads();                                   // (b)

    // ---- (c) per owned key tile: S, dP -> P, dS ; dV += P^T dO ; dK += dS^T Q ; park dS in LDS
#pragma unroll
    for (int t = 0; t < TPW; ++t) {
      const int key = (wave * TPW + t) * 16 + fr;
      const bool key_ok = key < p.M;
      Frag<T> pfrag, dsfrag;
#pragma unroll
      for (int qs = 0; qs < 2; ++qs) {
        f32x4 sacc = {0.f, 0.f, 0.f, 0.f}, pacc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int s = 0; s < 2; ++s) {
          mma16(sacc, qf[qs][s], kreg[t][s]);          // S[q = 16 qs + 4 fg + r][key]
          mma16(pacc, dof[qs][s], vreg[t][s]);         // dP
        }
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int ql = qs * 16 + 4 * fg + r;
          float pv = key_ok ? exp2f(sacc[r] * sl2 - sL[ql] * l2e) : 0.f;
          float dsv = pv * (pacc[r] - sD[ql]) * p.scale;
          pfrag.v[qs * 4 + r] = (T)pv;
          dsfrag.v[qs * 4 + r] = (T)dsv;
          sdS[ql * KS + key] = (T)dsv;
        }
      }
#pragma unroll
      for (int dt = 0; dt < 4; ++dt) {
        // B operands (n = d): k-slot (fg, j) <-> q = 16 (j>>2) + 4 fg + (j&3); re-read per tile to stay under 256 VGPRs
        const T* a = sQt + (dt * 16 + fr) * QS + 4 * fg;
        const T* c2 = sdOt + (dt * 16 + fr) * QS + 4 * fg;
        Frag<T> dotf = load_frag44<T>(c2, c2 + 16);
        Frag<T> qtf = load_frag44<T>(a, a + 16);
        mma16(dVacc[t][dt], pfrag, dotf);              // dV[key = tile*16 + 4 fg + r][d = 16 dt + fr]
        mma16(dKacc[t][dt], dsfrag, qtf);
      }
      __builtin_amdgcn_sched_barrier(0);
    }
    __syncthreads();                                   // (d)

    // ---- (e) dQ[32 x 64] = dS[32 x MP] K[MP x 64]: 8 output tiles (16 x 16) dealt round-robin to the waves
    for (int tile = wave; tile < 8; tile += NW) {
      const int qs = tile >> 2, dt = tile & 3;
      f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll 4
      for (int ks = 0; ks < MP / 32; ++ks) {
        Frag<T> a = load_frag8<T>(sdS + (qs * 16 + fr) * KS + 32 * ks + 8 * fg);
        Frag<T> bb = load_frag8<T>(sKt + (dt * 16 + fr) * KS + 32 * ks + 8 * fg);
        mma16(acc, a, bb);
      }
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        int q = q0 + qs * 16 + 4 * fg + r;
        if (q < q_end) dQg[(long)q * p.ldq + dt * 16 + fr] = (T)acc[r];
      }
    }
  }
  // ---- flush dK / dV
#pragma unroll
  for (int t = 0; t < TPW; ++t)
#pragma unroll
    for (int dt = 0; dt < 4; ++dt)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        int key = (wave * TPW + t) * 16 + 4 * fg + r;
        if (key < p.M) {
          if (nq_chunks == 1) {        // this workgroup saw every query of its (batch, head): the sums are final
            dKg[(long)key * p.lddkv + dt * 16 + fr] = dKacc[t][dt][r];
            dVg[(long)key * p.lddkv + dt * 16 + fr] = dVacc[t][dt][r];
          } else {
            atomicAdd(&dKg[(long)key * p.lddkv + dt * 16 + fr], dKacc[t][dt][r]);
            atomicAdd(&dVg[(long)key * p.lddkv + dt * 16 + fr], dVacc[t][dt][r]);
          }
        }
      }
}

}  // namespace

// ------------------------------------------------------------------------------------------------ plan -> launch
int mvlt_launch_attn_bwd(const mvlt_attn_bwd_args& a, const mvlt_attn_plan& p, hipStream_t s) {
  const char* const who = "mvlt_sr_attention_bwd";
#define BWD(NW, TPW) MVLT_ATTN_CASE((attn_bwd_kernel<float, NW, TPW>), (1, NW, TPW), p.nq_chunks, p.q_per_wg)
  switch (tkey(p.tp[0], p.tp[1], p.tp[2])) {
    BWD(4, 1) BWD(4, 2) BWD(4, 3) BWD(8, 2) BWD(6, 3)                                  // (bf16 is attn_bwd_dma_kernel's; fp32 past 288 keys streams)
  }
#undef BWD
  return attn_no_instantiation(who, p);
}
